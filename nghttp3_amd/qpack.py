"""QPACK field-line framing around the batch Huffman engine (SURVEY.md
section 8(f) rows 1-2), over the C-ABI of nghttp3_amd/csrc/qh_qpack.c.

* ``scan_field_section`` / ``scan_blocks`` / ``scan_encoder_stream`` --
  the framing of nghttp3_qpack_decoder_read_request
  (lib/nghttp3_qpack.c:3347-3800) and nghttp3_qpack_decoder_read_encoder
  (:2815-3150), returning field lines and (off, len, flags) string spans.
* ``write_indexed`` / ``write_indexed_name`` / ``write_literal`` -- the
  representation writers (qpack.c:1851-2069) with the reference's
  Huffman-iff-shorter choice.
* ``FieldSectionDecoder`` -- whole header blocks in, decoded strings out:
  host-side scan, then every Huffman string of the batch in one
  ``qh_decode_batch`` call on the GPU.

Error values are the reference's: -401 DECOMPRESSION_FAILED, -402
ENCODER_STREAM_ERROR, -109 HEADER_TOO_LARGE (nghttp3.h:224-259).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._arrays import Backend, cap_for, grow
from .qpack_huffman import SPAN_IN_DTYPE, SPAN_OUT_DTYPE, HuffmanBatchCodec

QH_ERR_QPACK_HEADER_TOO_LARGE = -109
QH_ERR_QPACK_DECOMPRESSION_FAILED = -401
QH_ERR_QPACK_ENCODER_STREAM_ERROR = -402
QH_ERR_QPACK_DECODER_STREAM_ERROR = -403

SPAN_HUFFMAN, SPAN_NAME = 0x1, 0x2
(FL_INDEXED, FL_INDEXED_PB, FL_INDEXED_NAME, FL_INDEXED_NAME_PB, FL_LITERAL,
 ES_INSERT_INDEXED, ES_INSERT, ES_SET_DTABLE_CAP, ES_DUPLICATE) = range(1, 10)
FL_DYNAMIC, FL_NEVER = 0x1, 0x2

FIELD_LINE_DTYPE = np.dtype([("index", "<u8"), ("opcode", "u1"), ("flags", "u1"),
                             ("reserved", "<u2"), ("name", "<i4"), ("value", "<i4"),
                             ("reserved2", "<u4")])
assert FIELD_LINE_DTYPE.itemsize == 24


PREFIX_DTYPE = np.dtype([("ricnt", "<u8"), ("delta_base", "<u8"), ("sign", "<u4"),
                         ("reserved", "<u4")])


# include/qhuff.h qh_field, qh_dyn_entry, qh_dtable_view
FIELD_DTYPE = np.dtype([("name_off", "<u8"), ("value_off", "<u8"), ("name_len", "<u4"),
                        ("value_len", "<u4"), ("token", "<i4"), ("name_where", "u1"),
                        ("value_where", "u1"), ("flags", "u1"), ("reserved", "u1")])
DYN_ENTRY_DTYPE = np.dtype([("name_off", "<u8"), ("value_off", "<u8"), ("name_len", "<u4"),
                            ("value_len", "<u4"), ("token", "<i4"), ("reserved", "<u4")])
ACCT_DTYPE = np.dtype([("hard_max", "<u8"), ("cap", "<u8"), ("size", "<u8"), ("reserved", "<u8")])
VIEW_DTYPE = np.dtype([("ent_base", "<i8"), ("live_lo", "<u8"), ("insert_count", "<u8"),
                       ("max_entries", "<u8"), ("reserved", "<u8")])
assert FIELD_DTYPE.itemsize == 32 and DYN_ENTRY_DTYPE.itemsize == 32 and VIEW_DTYPE.itemsize == 40
DYN_INDEX_REC_DTYPE = np.dtype([("ent_base", "<i8"), ("lo", "<u8"), ("hi", "<u8"), ("slot_off", "<u8"),
                                ("nbuckets", "<u4"), ("reserved", "<u4", (3,))])
DYN_KEY_DTYPE = np.dtype([("name_id", "<u4"), ("name_len", "<u4"), ("value_len", "<u4"),
                          ("value_hash", "<u4")])
assert DYN_KEY_DTYPE.itemsize == 16
ENC_INDEX_REC_DTYPE = np.dtype([("slot_off", "<u8"), ("hi", "<u8"), ("ring", "<u4"), ("nbuckets", "<u4"),
                                ("reserved", "<u8")])
assert ENC_INDEX_REC_DTYPE.itemsize == 32
ENC_STATE_DTYPE = np.dtype([("krcnt", "<u8"), ("pin_min", "<u8"), ("max_blocked", "<u8"),
                            ("nblocked", "<u8"), ("nstreams", "<u8"), ("flags", "<u8"),
                            ("min_update", "<u8"), ("last_update", "<u8")])
assert ENC_STATE_DTYPE.itemsize == 64
ENC_IMMEDIATE_ACK, ENC_STRAT_NONE, ENC_CAP_PENDING = 0x1, 0x2, 0x4
ENC_SEC_STREAM_BLOCKED, ENC_SEC_STREAM_KNOWN = 0x1, 0x2
NV_NEVER_INDEX, NV_TRY_INDEX = 0x1, 0x2
# include/qhuff.h qh_enc_ref, qh_enc_refs
ENC_REF_DTYPE = np.dtype([("stream_id", "<u8"), ("max_cnt", "<u8"), ("min_cnt", "<u8"),
                          ("reserved", "<u8")])
ENC_REFS_DTYPE = np.dtype([("base", "<u8"), ("n", "<u8"), ("dlen", "<u8"), ("flags", "<u8")])
assert ENC_REF_DTYPE.itemsize == 32 and ENC_REFS_DTYPE.itemsize == 32
ENC_REFS_BAD = 0x1
DEC_BLK_DTYPE = np.dtype([("stream_id", "<u8"), ("ricnt", "<u8"), ("off", "<u8"), ("len", "<u4"),
                          ("reserved", "<u4")])
DEC_BLKS_DTYPE = np.dtype([("base", "<u8"), ("n", "<u8"), ("max_blocked", "<u8"), ("flags", "<u8")])
assert DEC_BLK_DTYPE.itemsize == 32 and DEC_BLKS_DTYPE.itemsize == 32
# include/qhuff.h qh_dec_part, qh_dec_parts
DEC_PART_DTYPE = np.dtype([("stream_id", "<u8"), ("off", "<u8"), ("len", "<u4"), ("reserved0", "<u4"),
                           ("reserved1", "<u8")])
DEC_PARTS_DTYPE = np.dtype([("base", "<u8"), ("n", "<u8"), ("max_bytes", "<u8"), ("flags", "<u8")])
assert DEC_PART_DTYPE.itemsize == 32 and DEC_PARTS_DTYPE.itemsize == 32
PART_DONE, PART_KEPT = 0, 2
# include/qhuff.h qh_ustream
USTREAM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("held", "<u4"), ("ulen", "<u8"), ("flags", "<u4"),
                          ("reserved", "<u4")])
assert USTREAM_DTYPE.itemsize == 32
USTREAM_BAD, USTREAM_LATCH, USTREAM_MAX_ENCODERLEN = 0x1, 0x1, 131072
IN_SRC, IN_DST, IN_STATIC, IN_DYN, IN_OUT = range(5)
# include/qhuff.h qh_http_state, QH_HTTP_*
HTTP_STATE_DTYPE = np.dtype([("content_length", "<i8"), ("status_code", "<i4"), ("flags", "<u4")])
assert HTTP_STATE_DTYPE.itemsize == 16
HTTP_REQUEST, HTTP_TRAILERS, HTTP_CONNECT_PROTOCOL = 1, 2, 4
HTTP_KEEP, HTTP_REMOVE, HTTP_MALFORMED, HTTP_UNSEEN = range(4)
HTTP_NO_FIELD = 0xFFFFFFFF
QH_ERR_MALFORMED_HTTP_HEADER = -105
# include/qhuff.h qh_h3_stream, QH_H3_*
H3_STREAM_DTYPE = np.dtype([("left", "<u8"), ("acc", "<u8"), ("recv", "<i8"), ("state", "u1"), ("vleft", "u1"),
                            ("fclass", "u1"), ("hstate", "u1"), ("flags", "<u2"), ("err", "<i2")])
assert H3_STREAM_DTYPE.itemsize == 32
H3_OPEN, H3_END, H3_WAIT = 0, 1, 2
H3_ST_FRAME_TYPE, H3_ST_FRAME_LENGTH, H3_ST_DATA, H3_ST_HEADERS, H3_ST_IGN_FRAME, H3_ST_IGN_REST = range(6)
H3_RESPONSE, H3_PENDING, H3_SAW_DATA, H3_SAW_END = 0x1, 0x2, 0x4, 0x8
QH_ERR_MALFORMED_HTTP_MESSAGING = -107
QH_ERR_H3_FRAME_UNEXPECTED = -601
# include/qhuff.h qh_h3_item, qh_h3_tx, QH_H3W_*
H3_ITEM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("span_flags", "<u4"), ("type", "<u8"), ("src", "<u4"),
                          ("flags", "<u4")])
H3_TX_DTYPE = np.dtype([("off", "<u8"), ("flags", "<u4"), ("rsv", "<u4")])
assert H3_ITEM_DTYPE.itemsize == 32 and H3_TX_DTYPE.itemsize == 16
H3_FRAME_DATA, H3_FRAME_HEADERS = 0, 1
H3W_END = 0x1    # an item's flag: the stream ends after it
H3W_ENDED = 0x1  # a record's flag
QH_ERR_INVALID_STATE = -102
QH_ERR_H3_FRAME_ERROR = -602
QH_ERR_H3_GENERAL_PROTOCOL_ERROR = -606
# include/qhuff.h qh_h3_uni, qh_h3_conn, qh_h3_event, QH_H3U_*, QH_H3C_*, QH_H3_EV_*
H3_UNI_DTYPE = np.dtype([("left", "<u8"), ("acc", "<u8"), ("aux", "<u8"), ("state", "u1"), ("vleft", "u1"),
                         ("type", "u1"), ("ftype", "u1"), ("flags", "<u2"), ("err", "<i2")])
H3_CONN_DTYPE = np.dtype([("max_field_section_size", "<u8"), ("qpack_max_dtable_capacity", "<u8"),
                          ("qpack_blocked_streams", "<u8"), ("goaway_id", "<u8"), ("max_pushes", "<u8"),
                          ("max_client_streams", "<u8"), ("pri_buf", "u1", (8,)), ("pri_len", "u1"),
                          ("rsv", "u1"), ("flags", "<u2"), ("err", "<i2"), ("rsv2", "<u2")])
H3_EVENT_DTYPE = np.dtype([("kind", "<u4"), ("chunk", "<u4"), ("id", "<u8"), ("value", "u1", (8,)),
                           ("len", "<u4"), ("rsv", "<u4")])
H3_SETTINGS_DTYPE = np.dtype([("max_field_section_size", "<u8"), ("qpack_max_dtable_capacity", "<u8"),
                              ("qpack_blocked_streams", "<u8"), ("enable_connect_protocol", "u1"),
                              ("h3_datagram", "u1"), ("rsv", "u1", (6,))])
assert H3_UNI_DTYPE.itemsize == 32 and H3_CONN_DTYPE.itemsize == 64 and H3_EVENT_DTYPE.itemsize == 32
assert H3_SETTINGS_DTYPE.itemsize == 32
H3U_OPEN, H3U_GONE = 0, 1
(H3U_ST_FRAME_TYPE, H3U_ST_FRAME_LENGTH, H3U_ST_SETTINGS, H3U_ST_GOAWAY, H3U_ST_MAX_PUSH_ID, H3U_ST_IGN_FRAME,
 H3U_ST_SETTINGS_ID, H3U_ST_SETTINGS_VALUE, H3U_ST_PRIORITY_UPDATE_PRI_ELEM_ID, H3U_ST_PRIORITY_UPDATE) = range(10)
H3U_T_NONE, H3U_T_CONTROL, H3U_T_QENC, H3U_T_QDEC, H3U_T_UNKNOWN = range(5)
H3C_SETTINGS_RECVED, H3C_CONTROL_OPENED, H3C_QENC_OPENED, H3C_QDEC_OPENED = 0x1, 0x2, 0x4, 0x8
H3C_GOAWAY_RECVED, H3C_SERVER, H3C_CONNECT_PROTOCOL, H3C_H3_DATAGRAM = 0x20, 0x100, 0x200, 0x400
H3C_CAP_NEW, H3C_BLOCKED_NEW = 0x800, 0x1000
H3_EV_SETTINGS, H3_EV_GOAWAY, H3_EV_PRIORITY_UPDATE, H3_EV_STOP_SENDING = 1, 2, 3, 4
QH_ERR_H3_MISSING_SETTINGS = -603
QH_ERR_H3_CLOSED_CRITICAL_STREAM = -605
QH_ERR_H3_ID_ERROR = -607
QH_ERR_H3_SETTINGS_ERROR = -608
QH_ERR_H3_STREAM_CREATION_ERROR = -609
# include/qhuff.h qh_h3_smap, qh_h3_sent, qh_h3_gap, QH_H3D_*, QH_H3M_*, QH_H3S_*
H3_SMAP_DTYPE = np.dtype([("slot_off", "<u4"), ("nslots", "<u4"), ("rec_off", "<u4"), ("rec_cap", "<u4"),
                          ("gap_off", "<u4"), ("nlive", "<u4"), ("free_head", "<u4"), ("hiwater", "<u4"),
                          ("num_streams", "<u8"), ("max_stream_id_bidi", "<i8"), ("tx_goaway_id", "<u8"),
                          ("call", "<u4"), ("ngaps", "u1"), ("flags", "u1"), ("err", "<i2")])
H3_SENT_DTYPE = np.dtype([("stream_id", "<u8"), ("pri_buf", "u1", (8,)), ("next", "<u4"), ("call", "<u4"),
                          ("flags", "<u2"), ("pri_len", "u1"), ("rsv", "u1"), ("rsv2", "<u4")])
H3_GAP_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8")])
assert H3_SMAP_DTYPE.itemsize == 64 and H3_SENT_DTYPE.itemsize == 32 and H3_GAP_DTYPE.itemsize == 16
H3D_NONE, H3D_BIDI, H3D_BIDI_REJECTED, H3D_UNI, H3D_AGAIN = range(5)
H3D_NOTICE, H3D_SHUTDOWN = 0, 1
H3D_GAPS = 33
H3D_NOREC = 0xFFFFFFFF
H3D_HASH = 0x9E3779B97F4A7C15
H3M_SERVER, H3M_GOAWAY_QUEUED, H3M_SHUTDOWN_COMMENCED = 0x01, 0x40, 0x80
H3S_LIVE, H3S_READ_EOF, H3S_SHUT_RD, H3S_SERVER_PRIORITY_SET, H3S_PRIORITY_UPDATE_RECVED = 0x1, 0x20, 0x200, 0x400, 0x800
QH_ERR_STREAM_IN_USE = -104
QH_ERR_STREAM_NOT_FOUND = -110
QH_ERR_CONN_CLOSING = -111
EMIT_BLOCKED = 1
EMIT_QIF = 0x1


class qh_section_prefix(ctypes.Structure):
    _fields_ = [("ricnt", ctypes.c_uint64), ("delta_base", ctypes.c_uint64),
                ("sign", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class qh_plan_dyn(ctypes.Structure):
    """include/qhuff.h qh_plan_dyn (the table states of a planning call)."""
    _fields_ = [("views", ctypes.c_void_p), ("nviews", ctypes.c_size_t),
                ("section_view", ctypes.c_void_p), ("ref_limit", ctypes.c_void_p),
                ("dyn_entries", ctypes.c_void_p), ("nentries", ctypes.c_size_t),
                ("dyn_keys", ctypes.c_void_p), ("dyn_bytes", ctypes.c_void_p),
                ("nbytes", ctypes.c_uint64)]


class qh_plan_dyn_index(ctypes.Structure):
    """include/qhuff.h qh_plan_dyn_index (the index of a planning call)."""
    _fields_ = [("recs", ctypes.c_void_p), ("slots", ctypes.c_void_p), ("nslots", ctypes.c_uint64)]


class qh_h3d_tab(ctypes.Structure):
    """include/qhuff.h qh_h3d_tab (the state arrays of the stream-table calls)."""
    _fields_ = [("sm", ctypes.c_void_p), ("nconns", ctypes.c_size_t), ("slots", ctypes.c_void_p),
                ("nslots", ctypes.c_uint64), ("ents", ctypes.c_void_p), ("nrecs", ctypes.c_uint64),
                ("gaps", ctypes.c_void_p), ("ngaps", ctypes.c_uint64), ("rs_pool", ctypes.c_void_p),
                ("hs_pool", ctypes.c_void_p), ("us_pool", ctypes.c_void_p)]


# dispatch's lists: name -> bytes per arrival, in qh_h3d_lists' order (u_conn_start: per connection + 1)
H3D_LISTS = (("b_chunks", 16), ("b_fin", 1), ("b_sid", 8), ("b_view", 4), ("b_rec", 4), ("rs_call", 32),
             ("hs_call", 16), ("u_chunks", 16), ("u_fin", 1), ("u_sid", 8), ("u_rec", 4), ("u_conn_start", 4),
             ("us_call", 32))


class qh_h3d_lists(ctypes.Structure):
    """include/qhuff.h qh_h3d_lists (the outputs of a dispatch)."""
    _fields_ = [(name, ctypes.c_void_p) for name, _ in H3D_LISTS]


SECTIONS_DTABLE0 = 0x1


class qh_sections(ctypes.Structure):
    """include/qhuff.h qh_sections (outputs of qh_decode_sections_batch)."""
    _fields_ = [("lines", ctypes.c_void_p), ("lines_cap", ctypes.c_size_t),
                ("spans", ctypes.c_void_p), ("spans_cap", ctypes.c_size_t),
                ("strs", ctypes.c_void_p), ("verdict", ctypes.c_void_p),
                ("token", ctypes.c_void_p), ("line_start", ctypes.c_void_p),
                ("span_start", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("prefixes", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("dst_cap", ctypes.c_uint64),
                ("nlines", ctypes.c_uint64), ("nspans", ctypes.c_uint64),
                ("nhuff", ctypes.c_uint64), ("dst_need", ctypes.c_uint64)]


_L = None


def _pair(lib, stem, args):
    """A host twin qh_qpack_<stem>(args) and its batch form
    qh_<stem>_batch(ctx, args, where), declared together."""
    host, batch = getattr(lib, "qh_qpack_" + stem), getattr(lib, "qh_%s_batch" % stem)
    host.argtypes, batch.argtypes = args, [ctypes.c_void_p] + args + [ctypes.c_int]
    host.restype = batch.restype = ctypes.c_int


def _load():
    global _L
    if _L is None:
        lib = _lib.load()
        c = ctypes
        vp, sz, u64, u8, i32 = c.c_void_p, c.c_size_t, c.c_uint64, c.c_uint8, c.c_int
        lib.qh_qpack_scan_field_section.argtypes = [vp, sz, u64, c.POINTER(qh_section_prefix), vp, sz,
                                                    c.POINTER(sz), vp, sz, c.POINTER(sz)]
        lib.qh_qpack_scan_field_section.restype = i32
        lib.qh_qpack_scan_blocks.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp]
        lib.qh_qpack_scan_blocks.restype = i32
        lib.qh_qpack_scan_encoder_stream.argtypes = [vp, sz, u64, vp, sz, c.POINTER(sz), vp, sz,
                                                     c.POINTER(sz)]
        lib.qh_qpack_scan_encoder_stream.restype = c.c_ssize_t
        lib.qh_qpack_put_varint_len.argtypes = [u64, sz]
        lib.qh_qpack_put_varint_len.restype = sz
        lib.qh_qpack_put_varint.argtypes = [vp, u64, sz]
        lib.qh_qpack_put_varint.restype = vp
        lib.qh_qpack_write_indexed.argtypes = [vp, u8, u64, sz]
        lib.qh_qpack_write_indexed.restype = sz
        lib.qh_qpack_write_indexed_name.argtypes = [vp, u8, u64, sz, vp, sz]
        lib.qh_qpack_write_indexed_name.restype = sz
        lib.qh_qpack_write_literal.argtypes = [vp, u8, sz, vp, sz, vp, sz]
        lib.qh_qpack_write_literal.restype = sz
        lib.qh_qpack_literal_bound.argtypes = [sz, sz]
        lib.qh_qpack_literal_bound.restype = sz
        lib.qh_qpack_write_sections.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp]
        lib.qh_qpack_write_sections.restype = i32
        lib.nghttp3_check_header_name.argtypes = [vp, sz]
        lib.nghttp3_check_header_name.restype = i32
        lib.nghttp3_check_header_value.argtypes = [vp, sz]
        lib.nghttp3_check_header_value.restype = i32
        lib.qh_check_fields_batch.argtypes = [vp, vp, vp, sz, vp, i32]
        lib.qh_check_fields_batch.restype = i32
        lib.qh_scan_blocks_batch.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, sz,
                                             c.POINTER(c.c_uint64), i32]
        lib.qh_scan_blocks_batch.restype = i32
        lib.qh_qpack_lookup_token.argtypes = [vp, sz]
        lib.qh_qpack_lookup_token.restype = c.c_int32
        lib.qh_lookup_tokens_batch.argtypes = [vp, vp, vp, sz, vp, i32]
        lib.qh_lookup_tokens_batch.restype = i32
        lib.qh_decode_sections_batch.argtypes = [vp, vp, vp, sz, c.c_uint32, c.POINTER(qh_sections),
                                                 i32]
        lib.qh_decode_sections_batch.restype = i32
        lib.qh_qpack_static_entry.argtypes = [sz, c.POINTER(vp), c.POINTER(sz), c.POINTER(vp),
                                              c.POINTER(sz)]
        lib.qh_qpack_static_entry.restype = i32
        _pair(lib, "plan_fields", [vp, vp, sz, vp, vp])
        lib.qh_encode_sections_batch.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, vp, u64, vp,
                                                 c.POINTER(u64), i32]
        lib.qh_encode_sections_batch.restype = i32
        lib.qh_encode_fields_batch.argtypes = [vp, vp, vp, sz, vp, sz, vp, u64, vp, c.POINTER(u64), i32]
        lib.qh_encode_fields_batch.restype = i32
        _pair(lib, "dyn_keys", [vp, sz, vp, u64, sz, sz, vp])
        dynp = c.POINTER(qh_plan_dyn)
        _pair(lib, "plan_fields_dyn", [vp, vp, sz, vp, vp, sz, dynp, vp, vp, vp, vp])
        lib.qh_encode_fields_dyn_batch.argtypes = [vp, vp, vp, sz, vp, sz, dynp, vp, u64, vp,
                                                   c.POINTER(u64), vp, vp, i32]
        lib.qh_encode_fields_dyn_batch.restype = i32
        idxp = c.POINTER(qh_plan_dyn_index)
        _pair(lib, "dyn_index", [vp, sz, vp, sz, vp, sz, c.c_uint32, vp, vp, c.POINTER(u64), u64])
        _pair(lib, "plan_fields_dyn_indexed", [vp, vp, sz, vp, vp, sz, dynp, idxp, vp, vp, vp, vp])
        lib.qh_encode_fields_dyn_indexed_batch.argtypes = [vp, vp, vp, sz, vp, sz, dynp, idxp, vp, u64, vp,
                                                           c.POINTER(u64), vp, vp, i32]
        lib.qh_encode_fields_dyn_indexed_batch.restype = i32
        lib.qh_dtable_new.argtypes = [c.POINTER(vp), u64]
        lib.qh_dtable_new.restype = i32
        lib.qh_dtable_del.argtypes = [vp]
        lib.qh_dtable_del.restype = None
        lib.qh_dtable_apply.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        lib.qh_dtable_apply.restype = i32
        lib.qh_dtable_get_view.argtypes = [vp, vp]
        lib.qh_dtable_get_view.restype = i32
        lib.qh_dtable_entries.argtypes = [vp, c.POINTER(sz)]
        lib.qh_dtable_entries.restype = vp
        lib.qh_dtable_bytes.argtypes = [vp, c.POINTER(sz)]
        lib.qh_dtable_bytes.restype = vp
        _pair(lib, "emit_fields", [vp, vp, sz, c.POINTER(qh_sections), vp, vp, vp, vp, vp, sz, c.c_uint32,
                                   c.POINTER(_lib.qh_emit)])
        lib.qh_dtable_state_init.argtypes = [u64, vp, vp]
        lib.qh_dtable_state_init.restype = None
        pu64 = c.POINTER(u64)
        _pair(lib, "dtables_apply", [vp, vp, vp, sz, sz, vp, vp, vp, pu64, u64, vp, pu64, u64, vp, vp])
        _pair(lib, "dtables_compact", [sz, vp, vp, u64, vp, u64, vp, pu64, u64, vp, pu64, u64, vp])
        lib.qh_enc_state_init.argtypes = [u64, u64, u64, vp, vp, vp]
        lib.qh_enc_state_init.restype = None
        lib.qh_enc_state_set_capacity.argtypes = [vp, vp, u64]
        lib.qh_enc_state_set_capacity.restype = None
        _pair(lib, "encode_conns", [vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, pu64, u64,
                                    vp, pu64, u64, vp, vp, vp, vp, vp, vp, u64, vp, pu64, vp, u64, vp, pu64,
                                    vp])
        _pair(lib, "enc_index_init", [vp, vp, sz, vp, sz, vp, sz, u64, c.c_uint32, vp, vp, pu64, u64])
        _pair(lib, "encode_conns_indexed", [vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, pu64,
                                            u64, vp, pu64, u64, vp, vp, vp, vp, vp, vp, u64, vp, pu64, vp, u64,
                                            vp, pu64, vp, vp, vp, u64])
        lib.qh_enc_refs_init.argtypes = [vp]
        lib.qh_enc_refs_init.restype = None
        _pair(lib, "enc_sec_flags", [vp, sz, vp, sz, vp, sz, vp, vp, vp, u64, vp, vp])
        _pair(lib, "enc_refs_record", [vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, pu64, u64])
        _pair(lib, "enc_refs_compact", [vp, sz, sz, vp, vp, u64, vp, pu64, u64])
        _pair(lib, "enc_read_decoder", [vp, vp, vp, sz, sz, vp, vp, vp, vp, u64, vp, vp])
        _pair(lib, "dec_write_decoder", [vp, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, u64, vp, pu64])
        lib.qh_dec_blks_init.argtypes = [u64, vp]
        lib.qh_dec_blks_init.restype = None
        _pair(lib, "dec_blocked_push", [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, pu64, u64, vp, pu64, u64, vp])
        _pair(lib, "dec_blocked_release", [vp, sz, sz, vp, vp, vp, u64, vp, vp, vp, vp, vp, pu64, u64])
        _pair(lib, "dec_blocked_cancel", [vp, vp, sz, sz, vp, vp, u64, vp])
        _pair(lib, "dec_blocked_compact", [vp, sz, sz, vp, vp, u64, vp, u64, vp, pu64, u64, vp, pu64, u64])
        lib.qh_dec_parts_init.argtypes = [u64, vp]
        lib.qh_dec_parts_init.restype = None
        _pair(lib, "dec_partial_push", [vp, vp, vp, vp, vp, sz, sz, vp, vp, pu64, u64, vp, pu64, u64, vp, vp,
                                        u64, pu64, vp, vp, vp, pu64])
        _pair(lib, "dec_partial_cancel", [vp, vp, sz, sz, vp, vp, u64, vp])
        _pair(lib, "dec_partial_compact", [vp, sz, sz, vp, vp, u64, vp, u64, vp, pu64, u64, vp, pu64, u64])
        lib.qh_ustream_init.argtypes = [vp]
        lib.qh_ustream_init.restype = None
        _pair(lib, "ustream_join", [vp, vp, vp, sz, sz, u64, vp, vp, pu64, u64, vp, vp])
        _pair(lib, "ustream_keep", [vp, vp, vp, sz, sz, c.c_uint32, vp])
        _pair(lib, "ustream_sections", [vp, vp, sz, sz, vp])
        _pair(lib, "ustream_compact", [sz, vp, vp, u64, vp, pu64, u64])
        lib.qh_http_state_init.argtypes = [vp, sz]
        lib.qh_http_state_init.restype = None
        _pair(lib, "http_check", [vp, sz, vp, sz, vp, u64, vp, vp, vp, vp, vp, vp, vp, sz, vp])
        lib.qh_h3_stream_init.argtypes = [vp, sz, i32]
        lib.qh_h3_stream_init.restype = None
        _pair(lib, "h3_read", [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, pu64, vp, vp,
                               u64, pu64])
        _pair(lib, "h3_settle", [vp, vp, vp, sz, vp])
        lib.qh_h3_tx_init.argtypes = [vp, sz]
        lib.qh_h3_tx_init.restype = None
        lib.qh_h3_write_hd.argtypes = [vp, u64, u64]
        lib.qh_h3_write_hd.restype = vp
        lib.qh_h3_write_hd_len.argtypes = [u64, u64]
        lib.qh_h3_write_hd_len.restype = sz
        _pair(lib, "h3_write", [vp, vp, vp, vp, sz, vp, vp, u64, pu64, vp, vp, vp])
        lib.qh_h3_uni_init.argtypes = [vp, sz]
        lib.qh_h3_uni_init.restype = None
        lib.qh_h3_conn_init.argtypes = [vp, sz, i32, u64]
        lib.qh_h3_conn_init.restype = None
        _pair(lib, "h3_uni_read", [vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, pu64, vp, vp, pu64,
                                   vp, u64, pu64])
        _pair(lib, "h3_settings_apply", [vp, vp, sz, sz, vp, vp])
        lib.qh_h3_write_settings.argtypes = [vp, vp]
        lib.qh_h3_write_settings.restype = sz
        lib.qh_h3_smap_init.argtypes = [vp, sz, i32, vp, vp]
        lib.qh_h3_smap_init.restype = i32
        tabp = c.POINTER(qh_h3d_tab)
        _pair(lib, "h3_dispatch", [tabp, vp, vp, vp, sz, vp, vp, vp, c.POINTER(qh_h3d_lists), pu64, pu64])
        _pair(lib, "h3_commit", [tabp, vp, vp, vp, sz, vp, vp, sz, vp])
        _pair(lib, "h3_open", [tabp, vp, vp, sz, vp, vp, vp])
        _pair(lib, "h3_find", [tabp, vp, vp, sz, vp])
        _pair(lib, "h3_recs_move", [vp, u64, vp, vp, sz, c.c_uint32, i32])
        _pair(lib, "h3_close", [tabp, vp, sz, vp, vp, vp, vp, pu64, vp])
        _pair(lib, "h3_shutdown", [tabp, vp, sz, i32, vp, vp])
        _L = lib
    return _L


def _u8(data):
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) \
        else np.ascontiguousarray(data, dtype=np.uint8)
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint8)[:0]
    return a


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _plain(x):
    """Plaintext as a uint8 array; an empty one becomes one zero byte (the
    batch calls take no NULL plain)."""
    a = _u8(x)
    return a if a.size else np.zeros(1, dtype=np.uint8)


def _as(x, dtype):
    """None, or a contiguous array of dtype."""
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def scan_field_section(buf, base_off: int = 0):
    """One complete field section -> (status, (ricnt, sign, delta_base) or
    None, lines FIELD_LINE_DTYPE, spans SPAN_IN_DTYPE).  On an error there
    are no lines and the spans are the strings read before it."""
    lib = _load()
    src = _u8(buf)
    cap = src.size + 1  # every line and string takes at least one byte
    lines = np.zeros(cap, dtype=FIELD_LINE_DTYPE)
    spans = np.zeros(cap, dtype=SPAN_IN_DTYPE)
    pf = qh_section_prefix()
    nl, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rv = lib.qh_qpack_scan_field_section(_vp(src), src.size, base_off, ctypes.byref(pf), _vp(lines),
                                         cap, ctypes.byref(nl), _vp(spans), cap, ctypes.byref(ns))
    if rv != 0:
        return rv, None, lines[:0], spans[:ns.value]
    return 0, (pf.ricnt, pf.sign, pf.delta_base), lines[:nl.value], spans[:ns.value]


def scan_blocks(src, blocks):
    """Batch of field sections (blocks: SPAN_IN_DTYPE into src) ->
    (lines, spans, line_start, span_start, status)."""
    lib = _load()
    src = _u8(src)
    blocks = np.ascontiguousarray(blocks, dtype=SPAN_IN_DTYPE)
    nb = blocks.size
    cap = int(blocks["len"].sum(dtype=np.uint64)) + 1
    lines = np.zeros(cap, dtype=FIELD_LINE_DTYPE)
    spans = np.zeros(cap, dtype=SPAN_IN_DTYPE)
    ls = np.zeros(nb + 1, dtype=np.uint32)
    ss = np.zeros(nb + 1, dtype=np.uint32)
    st = np.zeros(max(nb, 1), dtype=np.int32)
    _lib.check(lib.qh_qpack_scan_blocks(_vp(src), _vp(blocks), nb, _vp(lines), cap, _vp(spans), cap,
                                        _vp(ls), _vp(ss), _vp(st)), "qh_qpack_scan_blocks")
    return lines[:ls[nb]], spans[:ss[nb]], ls, ss, st[:nb]


def scan_blocks_dev(codec: HuffmanBatchCodec, src, blocks, lines, spans, line_start, span_start,
                    status, huff=None):
    """GPU framing (qh_scan_blocks_batch) over torch tensors in HBM: src
    uint8, blocks int64 [n,2] (SPAN_IN layout), lines uint8 [cap*24], spans
    int64 [cap,2], line_start / span_start int32 [n+1], status int32 [n],
    optional huff int64 [cap,2] (the Huffman spans alone).  Returns the
    totals (lines, spans, Huffman spans)."""
    lib = _load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    tot = (ctypes.c_uint64 * 3)()
    _lib.check(lib.qh_scan_blocks_batch(codec._ctx, p(src), p(blocks), blocks.shape[0], p(lines),
                                        lines.numel() // FIELD_LINE_DTYPE.itemsize, p(spans),
                                        spans.shape[0], p(line_start), p(span_start), p(status),
                                        p(huff), 0 if huff is None else huff.shape[0], tot,
                                        _lib.QH_WHERE_DEVICE), "qh_scan_blocks_batch")
    return tot[0], tot[1], tot[2]


def scan_encoder_stream(buf, base_off: int = 0):
    """-> (consumed bytes or negative error, instructions, spans)."""
    lib = _load()
    src = _u8(buf)
    cap = src.size + 1
    lines = np.zeros(cap, dtype=FIELD_LINE_DTYPE)
    spans = np.zeros(cap, dtype=SPAN_IN_DTYPE)
    nl, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rv = lib.qh_qpack_scan_encoder_stream(_vp(src), src.size, base_off, _vp(lines), cap,
                                          ctypes.byref(nl), _vp(spans), cap, ctypes.byref(ns))
    return rv, lines[:nl.value], spans[:ns.value]


def put_varint(n: int, prefix: int, fb: int = 0) -> bytes:
    lib = _load()
    buf = (ctypes.c_uint8 * 16)(fb)
    end = lib.qh_qpack_put_varint(buf, n, prefix)
    k = end - ctypes.addressof(buf)
    assert k == lib.qh_qpack_put_varint_len(n, prefix)
    return bytes(buf[:k])


def _write(fn, *args, bound):
    buf = np.zeros(bound, dtype=np.uint8)
    n = fn(_vp(buf), *args)
    return buf[:n].tobytes()


def write_indexed(fb: int, idx: int, prefix: int) -> bytes:
    return _write(_load().qh_qpack_write_indexed, fb, idx, prefix, bound=16)


def write_indexed_name(fb: int, nameidx: int, prefix: int, value: bytes) -> bytes:
    """qpack_encoder_write_indexed_name (qpack.c:1851-1896)."""
    lib = _load()
    v = _u8(value)
    return _write(lib.qh_qpack_write_indexed_name, fb, nameidx, prefix, _vp(v), v.size,
                  bound=lib.qh_qpack_literal_bound(0, v.size))


def write_literal(fb: int, prefix: int, name: bytes, value: bytes) -> bytes:
    """qpack_encoder_write_literal (qpack.c:1944-2006)."""
    lib = _load()
    nm, v = _u8(name), _u8(value)
    return _write(lib.qh_qpack_write_literal, fb, prefix, _vp(nm), nm.size, _vp(v), v.size,
                  bound=lib.qh_qpack_literal_bound(nm.size, v.size))


def write_sections(plain, strs, lines, line_start, prefixes=None):
    """Batch writer (qh_qpack_write_sections): -> (dst uint8, sections
    SPAN_IN_DTYPE), every section with a zero prefix, or with prefixes[b]
    (PREFIX_DTYPE)."""
    lib = _load()
    plain = _u8(plain)
    strs = np.ascontiguousarray(strs, dtype=SPAN_IN_DTYPE)
    lines = np.ascontiguousarray(lines, dtype=FIELD_LINE_DTYPE)
    line_start = np.ascontiguousarray(line_start, dtype=np.uint32)
    nsec = line_start.size - 1
    cap = int(strs["len"].sum(dtype=np.uint64)) + 20 * lines.size + 20 * nsec + 1
    dst = np.zeros(cap, dtype=np.uint8)
    sections = np.zeros(max(nsec, 1), dtype=SPAN_IN_DTYPE)
    pf = _as(prefixes, PREFIX_DTYPE)
    _lib.check(lib.qh_qpack_write_sections(_vp(plain), _vp(strs), _vp(lines), _vp(line_start), nsec,
                                           None if pf is None else _vp(pf), _vp(dst), cap,
                                           _vp(sections)),
               "qh_qpack_write_sections")
    end = int(sections["off"][nsec - 1] + sections["len"][nsec - 1]) if nsec else 0
    return dst[:end], sections[:nsec]


def synth_field_sections(seed: int, nblocks: int, fields=(4, 20), namelen=(4, 24),
                         valuelen=(1, 128), alphabet: bytes | None = None):
    """Deterministic synthetic header blocks at dynamic table 0 (config 4's
    shape; the qifs corpus itself is not available offline): per block a
    uniform number of field lines, 30% indexed static, 40% static name
    reference + value, 30% literal name + value; names and values are
    alphabet-A text (nghttp3_amd/synth.py).  Returns (src, blocks, plain,
    strs, lines, line_start)."""
    from . import synth
    alphabet = alphabet or synth.ALPHABET_A
    rng = np.random.default_rng(seed)
    nf = rng.integers(fields[0], fields[1] + 1, nblocks)
    nl = int(nf.sum())
    op = rng.choice(np.array([FL_INDEXED, FL_INDEXED_NAME, FL_LITERAL], dtype=np.uint8),
                    p=[0.3, 0.4, 0.3], size=nl)
    has_name = op == FL_LITERAL
    has_value = op != FL_INDEXED
    nlen = rng.integers(namelen[0], namelen[1] + 1, nl) * has_name
    vlen = rng.integers(valuelen[0], valuelen[1] + 1, nl) * has_value
    # strings in line order: name (if any) then value (if any)
    per = np.stack([nlen, vlen], axis=1).reshape(-1)
    present = np.stack([has_name, has_value], axis=1).reshape(-1)
    slen = per[present].astype(np.uint32)
    sidx = np.cumsum(present) - 1
    strs = np.zeros(slen.size, dtype=SPAN_IN_DTYPE)
    strs["len"] = slen
    if slen.size:
        strs["off"][1:] = np.cumsum(slen.astype(np.uint64))[:-1]
    plain = synth.fill(seed, int(slen.sum(dtype=np.uint64)), alphabet)
    lines = np.zeros(nl, dtype=FIELD_LINE_DTYPE)
    lines["opcode"] = op
    lines["index"] = rng.integers(0, 99, nl) * (op != FL_LITERAL)
    lines["name"] = np.where(has_name, sidx.reshape(-1, 2)[:, 0], -1)
    lines["value"] = np.where(has_value, sidx.reshape(-1, 2)[:, 1], -1)
    line_start = np.zeros(nblocks + 1, dtype=np.uint32)
    line_start[1:] = np.cumsum(nf)
    src, blocks = write_sections(plain, strs, lines, line_start)
    return src, blocks, plain, strs, lines, line_start


def check_header_name(name) -> int:
    """nghttp3_check_header_name (lib/nghttp3_http.c:691-709)."""
    a = _u8(name)
    return _load().nghttp3_check_header_name(_vp(a), a.size)


def check_header_value(value) -> int:
    """nghttp3_check_header_value (lib/nghttp3_http.c:798-838)."""
    a = _u8(value)
    return _load().nghttp3_check_header_value(_vp(a), a.size)


def check_fields_host(codec: HuffmanBatchCodec, src, spans):
    """Batch validation of host strings on the GPU (qh_check_fields_batch):
    spans' QH_SPAN_NAME flag selects the name check.  -> int8 verdicts."""
    lib = _load()
    src = _u8(src)
    spans = np.ascontiguousarray(spans, dtype=SPAN_IN_DTYPE)
    v = np.zeros(max(spans.size, 1), dtype=np.int8)
    _lib.check(lib.qh_check_fields_batch(codec._ctx, _vp(src), _vp(spans), spans.size, _vp(v),
                                         _lib.QH_WHERE_HOST), "qh_check_fields_batch")
    return v[:spans.size]


def check_fields_dev(codec: HuffmanBatchCodec, src, spans, verdict):
    """Device-resident form: src uint8, spans int64 [n,2] (SPAN_IN layout),
    verdict int8 [n] torch tensors; asynchronous on the codec stream."""
    lib = _load()
    _lib.check(lib.qh_check_fields_batch(codec._ctx, ctypes.c_void_p(src.data_ptr()),
                                         ctypes.c_void_p(spans.data_ptr()), spans.shape[0],
                                         ctypes.c_void_p(verdict.data_ptr()), _lib.QH_WHERE_DEVICE),
               "qh_check_fields_batch")


def lookup_token(name) -> int:
    """qpack_lookup_token (lib/nghttp3_qpack.c:342): token or -1."""
    a = _u8(name)
    return _load().qh_qpack_lookup_token(_vp(a), a.size)


def lookup_tokens_host(codec: HuffmanBatchCodec, src, spans):
    """Batch token lookup on the GPU over host strings -> int32 tokens."""
    lib = _load()
    src = _u8(src)
    spans = np.ascontiguousarray(spans, dtype=SPAN_IN_DTYPE)
    t = np.zeros(max(spans.size, 1), dtype=np.int32)
    _lib.check(lib.qh_lookup_tokens_batch(codec._ctx, _vp(src), _vp(spans), spans.size, _vp(t),
                                          _lib.QH_WHERE_HOST), "qh_lookup_tokens_batch")
    return t[:spans.size]


def lookup_tokens_dev(codec: HuffmanBatchCodec, src, spans, token):
    """Device-resident form (torch tensors: uint8 src, int64 [n,2] spans,
    int32 [n] tokens); asynchronous on the codec stream."""
    lib = _load()
    _lib.check(lib.qh_lookup_tokens_batch(codec._ctx, ctypes.c_void_p(src.data_ptr()),
                                          ctypes.c_void_p(spans.data_ptr()), spans.shape[0],
                                          ctypes.c_void_p(token.data_ptr()), _lib.QH_WHERE_DEVICE),
               "qh_lookup_tokens_batch")


def _huffman_flags(spans):
    """bool per span: its QH_SPAN_HUFFMAN flag (one pass over the flags' low
    bytes; the two-pass `(flags & 1) != 0` is a visible part of a
    host-memory decode of millions of spans)."""
    assert SPAN_HUFFMAN == 1 and spans.dtype == SPAN_IN_DTYPE and spans.flags.c_contiguous
    low = spans.view(np.uint8).reshape(-1, SPAN_IN_DTYPE.itemsize)[:, SPAN_IN_DTYPE.fields["flags"][1]]
    return (low & np.uint8(1)).view(np.bool_)


class FieldSectionDecoder:
    """Whole header blocks -> every string of every block, decoded, checked
    and (names) tokenised, through one qh_decode_sections_batch call: GPU
    framing, the batch Huffman decoder, a failed Huffman string failing its
    block with -401 as read_request does (qpack.c:3604-3609, :3693-3698),
    the field name / value check and token lookup of every string.

    ``decode_blocks`` takes host arrays (the library stages them);
    ``decode_blocks_dev`` takes tensors already in HBM.  ``dtable0`` decodes
    as a decoder whose dynamic table capacity is 0 (config 4)."""

    def __init__(self, device: int = 0, codec: HuffmanBatchCodec | None = None,
                 dtable0: bool = False):
        self.codec = codec or HuffmanBatchCodec(device)
        self.opts = SECTIONS_DTABLE0 if dtable0 else 0
        self._spare = None  # the last decode_blocks result's arrays (_host_bufs)

    def decode_blocks_dev(self, src, blocks, bufs=None, packed=False, prefixes=False):
        """src uint8 and blocks int64 [n,2] (SPAN_IN layout) torch tensors in
        HBM.  Returns a dict of torch tensors (lines, spans, strs, verdict,
        tokens, line_start, span_start, status, dst) plus the totals
        (nlines, nspans, nhuff, dst_need); `bufs` (a previous result)
        reuses its allocations.  Asynchronous after the framing sync.
        The record arrays hold one line and one string per byte of src, and
        grow to the call's totals when blocks overlap and hold more.
        ``packed`` (QH_SECTIONS_PACKED): the decoded Huffman strings back to
        back in dst (dst_need: their bytes) instead of the slot layout; the
        call then also waits for the decode.  ``prefixes``: also every
        block's section prefix as encoded (uint8 [n * 24], PREFIX_DTYPE),
        which ``emit_fields_dev`` needs."""
        import torch
        dev = src.device
        n = blocks.shape[0]
        b = bufs or {}
        cap = int(src.numel()) + 1  # every line and string takes >= 1 byte
        if b.get("cap", -1) < cap or b.get("n", -1) < n:
            b = {"cap": cap, "n": n,
                 "lines": torch.empty(cap * FIELD_LINE_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                 "spans": torch.empty((cap, 2), dtype=torch.int64, device=dev),
                 "strs": torch.empty((cap, 2), dtype=torch.int64, device=dev),
                 "verdict": torch.empty(cap, dtype=torch.int8, device=dev),
                 "tokens": torch.empty(cap, dtype=torch.int32, device=dev),
                 "line_start": torch.empty(n + 1, dtype=torch.int32, device=dev),
                 "span_start": torch.empty(n + 1, dtype=torch.int32, device=dev),
                 "status": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                 "dst": torch.empty(64, dtype=torch.uint8, device=dev)}
        if prefixes and b.get("prefixes") is None:
            b["prefixes"] = torch.empty(max(b["n"], 1) * PREFIX_DTYPE.itemsize, dtype=torch.uint8,
                                        device=dev)
        opts = self.opts | (_lib.QH_SECTIONS_PACKED if packed else 0)
        if packed and b["dst"].numel() < cap * 8 // 5:  # (the bound that always suffices)
            b["dst"] = torch.empty(cap * 8 // 5, dtype=torch.uint8, device=dev)
        lib = _load()
        p = lambda t: t.data_ptr()
        cap = b["cap"]
        for _ in range(3):  # again only when the records or dst were too small
            st = qh_sections(p(b["lines"]), cap, p(b["spans"]), cap, p(b["strs"]), p(b["verdict"]),
                             p(b["tokens"]), p(b["line_start"]), p(b["span_start"]), p(b["status"]),
                             p(b["prefixes"]) if prefixes else None, p(b["dst"]),
                             b["dst"].numel(), 0, 0, 0, 0)
            rv = lib.qh_decode_sections_batch(self.codec._ctx, ctypes.c_void_p(src.data_ptr()),
                                              ctypes.c_void_p(blocks.data_ptr()), n, opts,
                                              ctypes.byref(st), _lib.QH_WHERE_DEVICE)
            if rv == _lib.QH_ERR_NOMEM and max(st.nlines, st.nspans) > cap:
                # (blocks that overlap hold more lines and strings than src has bytes)
                cap = b["cap"] = int(max(st.nlines, st.nspans))
                b["lines"] = torch.empty(cap * FIELD_LINE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                b["spans"] = torch.empty((cap, 2), dtype=torch.int64, device=dev)
                b["strs"] = torch.empty((cap, 2), dtype=torch.int64, device=dev)
                b["verdict"] = torch.empty(cap, dtype=torch.int8, device=dev)
                b["tokens"] = torch.empty(cap, dtype=torch.int32, device=dev)
                continue
            if rv == _lib.QH_ERR_NOMEM and st.dst_need > b["dst"].numel():
                b["dst"] = torch.empty(int(st.dst_need), dtype=torch.uint8, device=dev)
                continue
            _lib.check(rv, "qh_decode_sections_batch")
            break
        b.update({"nlines": st.nlines, "nspans": st.nspans, "nhuff": st.nhuff,
                  "dst_need": st.dst_need})
        return b

    _HOST_ARRAYS = (("lines", FIELD_LINE_DTYPE), ("spans", SPAN_IN_DTYPE), ("strs", SPAN_OUT_DTYPE),
                    ("verdict", np.int8), ("tokens", np.int32))

    @staticmethod
    def _host_empty(raw, key, count, dtype, pinned):
        """raw["arrays"][key] = an uninitialised array; raw["roots"][key] the
        object that owns its memory (every view handed out refers to it)."""
        dtype = np.dtype(dtype)
        if pinned:
            import torch
            t = torch.empty(max(count * dtype.itemsize, 1), dtype=torch.uint8, pin_memory=True)
            root = t.numpy()
            arr = root[:count * dtype.itemsize].view(dtype)
        else:
            root = arr = np.empty(count, dtype=dtype)
        raw["arrays"][key] = arr
        raw["roots"][key] = root
        del root, arr
        raw["refs0"] = FieldSectionDecoder._refs(raw)

    @staticmethod
    def _refs(raw):
        import sys
        return [sys.getrefcount(raw["roots"][k]) for k in sorted(raw["roots"])]

    @staticmethod
    def _released(raw):
        """Whether nothing but `raw` itself refers to its arrays any more (a
        result hands out views of them, and each view holds its root)."""
        return FieldSectionDecoder._refs(raw) == raw["refs0"]

    def _host_bufs(self, bufs, cap, n, dst_size, pinned):
        """The output arrays of decode_blocks: those of `bufs` (a previous
        result) when large enough, else the last call's when its result has
        been dropped, else new ones (uninitialised: a result only ever shows
        what the call wrote)."""
        raw = bufs.get("_raw") if bufs else None
        if raw is None and self._spare is not None and self._released(self._spare):
            raw = self._spare
        if raw is None or raw["pinned"] != pinned or raw["cap"] < cap or raw["n"] < n:
            raw = {"arrays": {}, "roots": {}, "cap": cap, "n": n, "pinned": pinned}
            for k, dt in self._HOST_ARRAYS:
                self._host_empty(raw, k, cap, dt, pinned)
            self._host_empty(raw, "line_start", n + 1, np.uint32, pinned)
            self._host_empty(raw, "span_start", n + 1, np.uint32, pinned)
            self._host_empty(raw, "status", max(n, 1), np.int32, pinned)
            self._host_empty(raw, "prefixes", max(n, 1), PREFIX_DTYPE, pinned)
            self._host_empty(raw, "dst", dst_size, np.uint8, pinned)
        if raw["arrays"]["dst"].size < dst_size:
            self._host_empty(raw, "dst", dst_size, np.uint8, pinned)
        return raw

    def decode_blocks(self, src, blocks, packed=False, bufs=None, pinned=False, prefixes=False):
        """Host arrays in and out: -> dict with lines, spans, strs
        (SPAN_OUT_DTYPE: Huffman strings in dst, raw strings in src),
        huffman (bool per span), verdict, tokens, line_start, span_start,
        status, dst (its first dst_need bytes).
        ``packed`` (QH_SECTIONS_PACKED): the decoded Huffman strings back to
        back in dst; dst is sized by the bound that always suffices, so the
        library pipelines the call over slices of blocks.  ``bufs`` (a
        previous result) has its arrays written again when they are large
        enough; ``pinned`` allocates the arrays in page-locked memory.  The
        arrays are allocated uninitialised, and those of the last result
        are taken again once that result has been dropped.  (``prefixes``:
        accepted for symmetry with decode_blocks_dev; the host result always
        holds them.)"""
        del prefixes
        lib = _load()
        src = _u8(src)
        if src.size == 0:
            src = np.zeros(1, dtype=np.uint8)
        blocks = np.ascontiguousarray(blocks, dtype=SPAN_IN_DTYPE)
        n = blocks.size
        nbytes = int(blocks["len"].sum(dtype=np.uint64))
        cap = nbytes + 1
        # slots: a first guess (about twice the decoded bytes for header
        # text), grown to dst_need when short
        dst_size = max(nbytes * 8 // 5, 64) if packed else 3 * nbytes + 64
        raw = self._host_bufs(bufs, cap, n, dst_size, pinned)
        self._spare = None
        a = raw["arrays"]
        opts = self.opts | (_lib.QH_SECTIONS_PACKED if packed else 0)
        for _ in range(2):
            dst = a["dst"]
            st = qh_sections(a["lines"].ctypes.data, raw["cap"], a["spans"].ctypes.data, raw["cap"],
                             a["strs"].ctypes.data, a["verdict"].ctypes.data, a["tokens"].ctypes.data,
                             a["line_start"].ctypes.data, a["span_start"].ctypes.data,
                             a["status"].ctypes.data, a["prefixes"].ctypes.data, dst.ctypes.data,
                             dst.size, 0, 0, 0, 0)
            rv = lib.qh_decode_sections_batch(self.codec._ctx, _vp(src), _vp(blocks), n, opts,
                                              ctypes.byref(st), _lib.QH_WHERE_HOST)
            if rv == _lib.QH_ERR_NOMEM and st.dst_need > dst.size:
                del dst
                self._host_empty(raw, "dst", int(st.dst_need), np.uint8, pinned)
                continue
            _lib.check(rv, "qh_decode_sections_batch")
            break
        ns = int(st.nspans)
        spans = a["spans"][:ns]
        res = {"lines": a["lines"][:st.nlines], "spans": spans, "strs": a["strs"][:ns],
               "huffman": _huffman_flags(spans), "verdict": a["verdict"][:ns],
               "tokens": a["tokens"][:ns], "line_start": a["line_start"][:n + 1],
               "span_start": a["span_start"][:n + 1], "status": a["status"][:n],
               "prefixes": a["prefixes"][:n], "dst": dst[:int(st.dst_need)],
               "nlines": int(st.nlines), "nspans": ns, "nhuff": int(st.nhuff),
               "dst_need": int(st.dst_need), "_raw": raw}
        del dst, spans
        self._spare = raw
        return res


    # ---- field emission (qh_qpack_emit_fields / qh_emit_fields_batch) ----

    @staticmethod
    def _sections_struct(res, ptr):
        """The qh_sections of a finished decode result (its pointers through
        `ptr`)."""
        if res.get("prefixes") is None:
            raise ValueError("emit_fields needs a result decoded with prefixes=True")
        n = lambda k: ptr(res[k]) if res.get(k) is not None else None
        return qh_sections(n("lines"), int(res["nlines"]), n("spans"), int(res["nspans"]), n("strs"),
                           n("verdict"), n("tokens"), n("line_start"), n("span_start"), n("status"),
                           n("prefixes"), n("dst"), 0, int(res["nlines"]), int(res["nspans"]),
                           int(res["nhuff"]), int(res["dst_need"]))

    @staticmethod
    def _emit(be, addr, what, o, nl, materialise, call):
        """The emit call over the outputs `o` (room for nl fields), made once
        more with an ``out`` of out_need bytes when that was short -> qh_emit."""
        for _ in range(2):
            out = o["out"] if materialise else None
            e = _lib.qh_emit(addr(o["fields"]), nl, addr(o["field_start"]), addr(o["status"]),
                             addr(o["ricnt"]), addr(out) if materialise else None, be.size(out),
                             addr(o["out_blocks"]), 0, 0, 0)
            rv = call(ctypes.byref(e))
            if rv == _lib.QH_ERR_NOMEM and materialise and e.out_need > be.size(out):
                o["out"] = be.empty(int(e.out_need))
                continue
            _lib.check(rv, what)
            break
        return e

    @staticmethod
    def emit_fields(res, src, blocks, table=None, views=None, block_view=None, sel=None,
                    qif=False, materialise=True, entries=None, dyn_bytes=None):
        """Host arrays: the header list of every selected block of `res` (a
        decode_blocks result over src, blocks), indices resolved against the
        static table and `table` (a DynamicTable: its current state) or
        `views` (VIEW_DTYPE; block b decodes against views[block_view[b]],
        views[0] without block_view; entries / dyn_bytes default to
        table's).  -> dict: fields (FIELD_DTYPE), field_start, status (0,
        EMIT_BLOCKED, -401, -109), ricnt, out and out_blocks (materialise:
        the names and values back to back, QIF text with ``qif``), nfields,
        out_need, nblocked.  Runs on the host (qh_qpack_emit_fields; no
        context or GPU is involved, hence a static method)."""
        lib = _load()
        src = _u8(src)
        blocks = np.ascontiguousarray(blocks, dtype=SPAN_IN_DTYPE)
        if table is not None:
            views = table.view() if views is None else views
            entries, dyn_bytes = table.entries(), table.bytes()
        vw = None if views is None else _as(views, VIEW_DTYPE).reshape(-1)
        bv = _as(block_view, np.uint32)
        sl = _as(sel, np.uint32)
        ents = _as(entries, DYN_ENTRY_DTYPE)
        dbytes = None if dyn_bytes is None else _u8(dyn_bytes)
        nsel = blocks.size if sl is None else sl.size
        st = FieldSectionDecoder._sections_struct(res, lambda a: a.ctypes.data)
        o = {"fields": np.zeros(max(int(res["nlines"]), 1), dtype=FIELD_DTYPE),
             "field_start": np.zeros(nsel + 1, dtype=np.uint32),
             "status": np.zeros(max(nsel, 1), dtype=np.int32),
             "ricnt": np.zeros(max(nsel, 1), dtype=np.uint64),
             "out_blocks": np.zeros(max(nsel, 1), dtype=SPAN_IN_DTYPE),
             "out": np.zeros(1, dtype=np.uint8) if materialise else None}
        opt = lambda a: None if a is None else _vp(a)
        e = FieldSectionDecoder._emit(
            Backend(), lambda a: a.ctypes.data, "qh_qpack_emit_fields", o, o["fields"].size, materialise,
            lambda pe: lib.qh_qpack_emit_fields(_vp(src), _vp(blocks), blocks.size, ctypes.byref(st),
                                                opt(vw), opt(bv), opt(ents), opt(dbytes), opt(sl), nsel,
                                                EMIT_QIF if qif else 0, pe))
        return {"fields": o["fields"][:e.nfields], "field_start": o["field_start"],
                "status": o["status"][:nsel], "ricnt": o["ricnt"][:nsel],
                "out_blocks": o["out_blocks"][:nsel],
                "out": o["out"][:e.out_need] if materialise else None,
                "nfields": int(e.nfields), "out_need": int(e.out_need), "nblocked": int(e.nblocked)}

    def emit_fields_dev(self, res, src, blocks, table=None, views=None, block_view=None, sel=None,
                        qif=False, materialise=True, entries=None, dyn_bytes=None, bufs=None):
        """Device-resident form (qh_emit_fields_batch): `res` a
        decode_blocks_dev(..., prefixes=True) result over the torch tensors
        src, blocks.  `table` is a DynamicTable (uploaded with to_device: only
        the tail since the last upload crosses) or views / entries /
        dyn_bytes / block_view / sel are torch tensors already in HBM (views
        uint8 [nviews * 40], entries uint8 [n * 32], block_view and sel
        int32).  -> dict of torch tensors (fields uint8 [nfields * 32],
        field_start int32, status int32, ricnt int64, out uint8, out_blocks
        int64 [nsel, 2]) plus nfields, out_need, nblocked; `bufs` (a previous
        result) reuses its allocations.  One host wait, for the totals."""
        import torch
        lib = _load()
        dev = src.device
        if table is not None:
            d = table.to_device(dev)
            views = d["views"] if views is None else views
            entries, dyn_bytes = d["entries"], d["bytes"]
        n = blocks.shape[0]
        nsel = n if sel is None else sel.shape[0]
        nl = max(int(res["nlines"]), 1)
        b = bufs or {}
        if b.get("nl", -1) < nl or b.get("nsel", -1) < nsel:
            b = {"nl": nl, "nsel": nsel,
                 "fields": torch.empty(nl * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                 "field_start": torch.empty(nsel + 1, dtype=torch.int32, device=dev),
                 "status": torch.empty(max(nsel, 1), dtype=torch.int32, device=dev),
                 "ricnt": torch.empty(max(nsel, 1), dtype=torch.int64, device=dev),
                 "out_blocks": torch.empty((max(nsel, 1), 2), dtype=torch.int64, device=dev),
                 "out": torch.empty(64, dtype=torch.uint8, device=dev)}
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        st = self._sections_struct(res, lambda t: t.data_ptr())
        e = self._emit(
            Backend(dev), lambda t: t.data_ptr(), "qh_emit_fields_batch", b, b["nl"], materialise,
            lambda pe: lib.qh_emit_fields_batch(self.codec._ctx, p(src), p(blocks), n, ctypes.byref(st),
                                                p(views), p(block_view), p(entries), p(dyn_bytes),
                                                p(sel), nsel, EMIT_QIF if qif else 0, pe,
                                                _lib.QH_WHERE_DEVICE))
        b.update({"nfields": int(e.nfields), "out_need": int(e.out_need),
                  "nblocked": int(e.nblocked)})
        return b


    # ---- sections as HTTP messages (qh_qpack_http_check / qh_http_check_batch) ----

    @staticmethod
    def _http_check(be, fields, nfields, field_start, nsec, out, nout, emit_status, kind, states, o,
                    kept_cap=None, codec=None):
        """The call over the arrays of backend `be` -> rv.  `o`: the outputs
        fverdict, status, bad_field, kept, kept_start (bad_field and the kept
        pair may be None); kept_cap defaults to kept's room in records."""
        kept = o.get("kept")
        if kept_cap is None:
            kept_cap = be.size(kept) // FIELD_DTYPE.itemsize
        return be.call(_load(), "http_check", be.ptr(fields), nfields, be.ptr(field_start), nsec,
                       be.ptr(out), nout, be.ptr(emit_status), be.ptr(kind), be.ptr(states),
                       be.ptr(o["fverdict"]), be.ptr(o["status"]), be.ptr(o.get("bad_field")),
                       be.ptr(kept), kept_cap, be.ptr(o.get("kept_start")), codec=codec)

    @staticmethod
    def check_http(emit_result, kind, states, keep=True):
        """Host arrays: every section of an emit_fields(..., materialise=True)
        result judged as conn_decode_headers judges it (nghttp3_http_on_header
        per field, the end-of-headers check per section).  kind: one byte per
        section (HTTP_REQUEST or 0 for a response, | HTTP_TRAILERS, |
        HTTP_CONNECT_PROTOCOL); states: HTTP_STATE_DTYPE records
        (``http_states``), section p's at p, updated in place where the
        section passes.  -> dict: fverdict (int8 per field: HTTP_KEEP, _REMOVE,
        _MALFORMED, _UNSEEN), status (0, -105, or the skipped section's),
        bad_field, and with ``keep`` kept (FIELD_DTYPE: what recv_header would
        receive) and kept_start.  Runs on the host (qh_qpack_http_check)."""
        e = emit_result
        if e.get("out") is None:
            raise ValueError("check_http needs an emit result made with materialise=True")
        nf, fs = int(e["nfields"]), np.ascontiguousarray(e["field_start"], np.uint32)
        nsec = fs.size - 1
        kind = np.ascontiguousarray(kind, np.uint8)
        if kind.size != nsec or states.dtype != HTTP_STATE_DTYPE or states.size != nsec or \
                not states.flags.c_contiguous:
            raise ValueError("check_http: one kind byte and one state record per section")
        fields = np.ascontiguousarray(e["fields"], FIELD_DTYPE)
        out = _u8(e["out"])
        o = {"fverdict": np.zeros(nf, np.int8), "status": np.zeros(nsec, np.int32),
             "bad_field": np.zeros(nsec, np.uint32),
             "kept": np.zeros(max(nf, 1), FIELD_DTYPE).view(np.uint8) if keep else None,
             "kept_start": np.zeros(nsec + 1, np.uint32) if keep else None}
        be = Backend()
        st = None if e.get("status") is None else np.ascontiguousarray(e["status"], np.int32)
        rv = FieldSectionDecoder._http_check(be, fields.view(np.uint8), nf, fs, nsec, out, out.size, st,
                                             kind, states.view(np.uint8), o, kept_cap=nf)
        be.check(rv, "http_check")
        if keep:
            o["kept"] = o["kept"].view(FIELD_DTYPE)[:int(o["kept_start"][nsec])]
        o["states"] = states
        return o

    def check_http_dev(self, emit_result, kind, states, keep=True, bufs=None):
        """Device-resident form (qh_http_check_batch): `emit_result` an
        emit_fields_dev(..., materialise=True) result, kind a uint8 tensor
        [nsec], states a uint8 tensor [nsec * 16] (``http_states`` uploaded),
        updated in place.  -> dict of torch tensors (fverdict int8, status and
        bad_field and kept_start int32, kept uint8 [nfields * 32]); `bufs` (a
        previous result) reuses its allocations.  Asynchronous on the
        context's stream: no host wait."""
        import torch
        e = emit_result
        nf, nsec = int(e["nfields"]), int(kind.shape[0])
        dev = kind.device
        b = bufs or {}
        if b.get("nf", -1) < nf or b.get("nsec", -1) < nsec or (keep and b.get("kept") is None):
            b = {"nf": nf, "nsec": nsec,
                 "fverdict": torch.empty(max(nf, 1), dtype=torch.int8, device=dev),
                 "status": torch.empty(max(nsec, 1), dtype=torch.int32, device=dev),
                 "bad_field": torch.empty(max(nsec, 1), dtype=torch.int32, device=dev),
                 "kept": torch.empty(max(nf, 1) * FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                 if keep else None,
                 "kept_start": torch.empty(nsec + 1, dtype=torch.int32, device=dev) if keep else None}
        o = b if keep else dict(b, kept=None, kept_start=None)
        be = Backend(dev)
        rv = self._http_check(be, e["fields"], nf, e["field_start"], nsec, e["out"], int(e["out_need"]),
                              e.get("status"), kind, states, o, kept_cap=b["nf"] if keep else 0,
                              codec=self.codec)
        be.check(rv, "http_check")
        b["states"] = states
        return b


def http_states(n: int):
    """n fresh HTTP_STATE_DTYPE records (-1 / -1 / 0, qh_http_state_init)."""
    st = np.zeros(n, dtype=HTTP_STATE_DTYPE)
    if n:
        _load().qh_http_state_init(_vp(st), n)
    return st


# ---- request streams as they arrive (qh_qpack_h3_read / qh_h3_read_batch, _settle) ----

def h3_streams(n: int, response: bool = False):
    """n fresh H3_STREAM_DTYPE records (qh_h3_stream_init): the type state and
    REQ_INITIAL, or RESP_INITIAL with H3_RESPONSE for a client reading
    responses."""
    rs = np.zeros(n, dtype=H3_STREAM_DTYPE)
    if n:
        _load().qh_h3_stream_init(_vp(rs), n, 1 if response else 0)
    return rs


# The outputs of a read: name -> bytes per chunk (dspan_start has one entry more).
_H3_OUT = (("status", 4), ("consumed", 4), ("nunknown", 4), ("pieces", 16), ("piece_sid", 8),
           ("piece_view", 4), ("piece_fin", 1), ("piece_kind", 1))


def h3_read_raw(be, src, chunks, chunk_fin, chunk_sid, chunk_view, nchunks, rs, hs, o, dspan_cap,
                codec=None):
    """The call over byte arrays of backend `be` -> (rv, npieces, ndspans).
    `o`: the outputs of _H3_OUT plus dspan_start and dspans (nunknown and
    dspans may be None); dspan_cap the room of dspans in spans."""
    np_, nd = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rv = be.call(_load(), "h3_read", be.ptr(src), be.ptr(chunks), be.ptr(chunk_fin), be.ptr(chunk_sid),
                 be.ptr(chunk_view), nchunks, be.ptr(rs), be.ptr(hs), be.ptr(o["status"]),
                 be.ptr(o["consumed"]), be.ptr(o.get("nunknown")), be.ptr(o["pieces"]),
                 be.ptr(o["piece_sid"]), be.ptr(o["piece_view"]), be.ptr(o["piece_fin"]),
                 be.ptr(o["piece_kind"]), ctypes.byref(np_), be.ptr(o["dspan_start"]),
                 be.ptr(o.get("dspans")), dspan_cap, ctypes.byref(nd), codec=codec)
    return rv, int(np_.value), int(nd.value)


def _h3_read(be, src, chunks, chunk_fin, chunk_sid, chunk_view, n, rs, hs, bufs, codec=None):
    b = bufs or {}
    if b.get("n", -1) < n:
        b = {"n": n, "dspan_cap": b.get("dspan_cap", 0), "dspans": b.get("dspans")}
        for name, unit in _H3_OUT:
            b[name] = be.empty(max(n, 1) * unit)
        b["dspan_start"] = be.empty((n + 1) * 8)
    if b["dspans"] is None:
        b["dspan_cap"] = cap_for(n, 64)
        b["dspans"] = be.empty(b["dspan_cap"] * 16)

    def attempt():
        rv, npieces, nd = h3_read_raw(be, src, chunks, chunk_fin, chunk_sid, chunk_view, n, rs, hs, b,
                                      b["dspan_cap"], codec=codec)
        return rv, (npieces, nd)

    def more(needs):
        b["dspan_cap"] = cap_for(needs[1], 64)
        b["dspans"] = be.empty(b["dspan_cap"] * 16)

    _, (b["npieces"], b["ndspans"]) = be.retry("h3_read", attempt, more)
    return b


def h3_read(src, chunks, chunk_fin, chunk_sid, chunk_view, rs, hs):
    """Host arrays: the new bytes of many request streams cut into HTTP/3
    frames as nghttp3_conn_read_bidi cuts them.  chunks: SPAN_IN_DTYPE spans
    into src, one per stream, with chunk_fin (uint8), chunk_sid (uint64) and
    chunk_view (uint32); rs: H3_STREAM_DTYPE records (``h3_streams``), updated
    in place; hs: HTTP_STATE_DTYPE records (``http_states``), read only.  ->
    dict: status (H3_OPEN, H3_END, H3_WAIT or the error), consumed, nunknown per
    chunk; pieces (SPAN_IN_DTYPE), piece_sid, piece_view, piece_fin, piece_kind
    of the npieces HEADERS pieces, as qh_dec_partial_push takes them; dspans
    (SPAN_IN_DTYPE) and dspan_start (uint64, one entry more than chunks): the
    body spans.  Runs on the host (qh_qpack_h3_read)."""
    src = _u8(src)
    chunks = np.ascontiguousarray(chunks, SPAN_IN_DTYPE)
    n = chunks.size
    fin, sid = np.ascontiguousarray(chunk_fin, np.uint8), np.ascontiguousarray(chunk_sid, np.uint64)
    view = np.ascontiguousarray(chunk_view, np.uint32)
    if fin.size != n or sid.size != n or view.size != n or rs.dtype != H3_STREAM_DTYPE or rs.size != n or \
            hs.dtype != HTTP_STATE_DTYPE or hs.size != n or not rs.flags.c_contiguous:
        raise ValueError("h3_read: one fin, sid, view, stream record and HTTP state per chunk")
    hs = np.ascontiguousarray(hs)
    be = Backend()
    b = _h3_read(be, src, chunks.view(np.uint8), fin, sid.view(np.uint8), view.view(np.uint8), n,
                 rs.view(np.uint8), hs.view(np.uint8), None)
    npieces, nd = b["npieces"], b["ndspans"]
    return {"status": b["status"].view(np.int32)[:n], "consumed": b["consumed"].view(np.uint32)[:n],
            "nunknown": b["nunknown"].view(np.uint32)[:n], "npieces": npieces, "ndspans": nd,
            "pieces": b["pieces"].view(SPAN_IN_DTYPE)[:npieces],
            "piece_sid": b["piece_sid"].view(np.uint64)[:npieces],
            "piece_view": b["piece_view"].view(np.uint32)[:npieces],
            "piece_fin": b["piece_fin"][:npieces], "piece_kind": b["piece_kind"][:npieces],
            "dspan_start": b["dspan_start"].view(np.uint64), "dspans": b["dspans"].view(SPAN_IN_DTYPE)[:nd],
            "rs": rs}


def h3_read_dev(codec: HuffmanBatchCodec, src, chunks, chunk_fin, chunk_sid, chunk_view, rs, hs, bufs=None):
    """Device-resident form (qh_h3_read_batch): uint8 tensors holding the same
    records (chunks [n * 16], chunk_fin [n], chunk_sid [n * 8], chunk_view
    [n * 4], rs [n * 32] updated in place, hs [n * 16]).  -> dict of uint8
    tensors named as h3_read's arrays, with room for n chunks (the first
    npieces / ndspans entries are written), plus the host integers npieces and
    ndspans; `bufs` (a previous result) reuses its allocations.  One host wait,
    for the two totals."""
    n = int(chunk_fin.shape[0])
    return _h3_read(Backend(chunk_fin.device), src, chunks, chunk_fin, chunk_sid, chunk_view, n, rs, hs,
                    bufs, codec=codec)


def h3_settle(rs, hs, sec_status=None):
    """Host arrays: the records of the streams whose section the HTTP check
    has judged, settled in place (hs now includes the section; sec_status the
    check's status per stream, None: all 0).  -> status (int32: 0, H3_END or
    the error).  Runs on the host (qh_qpack_h3_settle)."""
    n = rs.size
    if rs.dtype != H3_STREAM_DTYPE or hs.dtype != HTTP_STATE_DTYPE or hs.size != n or \
            not rs.flags.c_contiguous:
        raise ValueError("h3_settle: one HTTP state per stream record")
    st = None if sec_status is None else np.ascontiguousarray(sec_status, np.int32)
    if st is not None and st.size != n:
        raise ValueError("h3_settle: one section status per stream record")
    status = np.zeros(n, np.int32)
    be = Backend()
    hs = np.ascontiguousarray(hs)
    rv = be.call(_load(), "h3_settle", be.ptr(rs.view(np.uint8)), be.ptr(hs.view(np.uint8)),
                 None if st is None else be.ptr(st.view(np.uint8)), n, be.ptr(status.view(np.uint8)))
    be.check(rv, "h3_settle")
    return status


def h3_settle_dev(codec: HuffmanBatchCodec, rs, hs, sec_status, status):
    """Device-resident form (qh_h3_settle_batch): rs a uint8 tensor [n * 32]
    updated in place, hs uint8 [n * 16], sec_status int32 [n] or None, status
    int32 [n] filled.  Asynchronous on the context's stream: no host wait."""
    n = int(status.shape[0])
    be = Backend(status.device)
    rv = be.call(_load(), "h3_settle", be.ptr(rs), be.ptr(hs), be.ptr(sec_status), n, be.ptr(status),
                 codec=codec)
    be.check(rv, "h3_settle")
    return status


# ---- response and request streams as they leave (qh_qpack_h3_write / qh_h3_write_batch) ----

def h3_tx(n: int):
    """n fresh H3_TX_DTYPE records (qh_h3_tx_init): offset 0, not ended."""
    tx = np.zeros(n, dtype=H3_TX_DTYPE)
    if n:
        _load().qh_h3_tx_init(_vp(tx), n)
    return tx


def h3_write_hd(type_: int, length: int) -> bytes:
    """The frame header nghttp3_frame_write_hd writes (qh_h3_write_hd; its
    length is qh_h3_write_hd_len)."""
    lib = _load()
    buf = np.zeros(16, np.uint8)
    n = lib.qh_h3_write_hd_len(type_, length)
    end = lib.qh_h3_write_hd(_vp(buf), type_, length)
    assert end - buf.ctypes.data == n
    return buf[:n].tobytes()


# The per-stream outputs of a write: name -> bytes per stream.
_H3W_OUT = (("out", 16), ("fin", 1), ("status", 4))


def h3_write_raw(be, hsrc, dsrc, items, item_start, nstreams, tx, dst, dst_cap, o, codec=None):
    """The call over byte arrays of backend `be` -> (rv, dst_need).  `o`: the
    outputs of _H3W_OUT; dst may be None (with dst_cap 0: the sizing call)."""
    need = ctypes.c_uint64(0)
    rv = be.call(_load(), "h3_write", be.ptr(hsrc), be.ptr(dsrc), be.ptr(items), be.ptr(item_start), nstreams,
                 be.ptr(tx), be.ptr(dst), dst_cap, ctypes.byref(need), be.ptr(o["out"]), be.ptr(o["fin"]),
                 be.ptr(o["status"]), codec=codec)
    return rv, int(need.value)


def _h3_write(be, hsrc, dsrc, items, item_start, n, tx, bufs, codec=None):
    b = bufs or {}
    if b.get("n", -1) < n:
        b = {"n": n, "dst_cap": b.get("dst_cap", 0), "dst": b.get("dst")}
        for name, unit in _H3W_OUT:
            b[name] = be.empty(max(n, 1) * unit)
    if b["dst"] is None:
        b["dst_cap"] = cap_for(be.size(hsrc) + be.size(dsrc) + 4 * n, 4096)
        b["dst"] = be.empty(b["dst_cap"])

    def attempt():
        rv, need = h3_write_raw(be, hsrc, dsrc, items, item_start, n, tx, b["dst"], b["dst_cap"], b, codec=codec)
        return rv, need

    def more(need):
        b["dst_cap"] = cap_for(need, 4096)
        b["dst"] = be.empty(b["dst_cap"])

    _, b["dst_need"] = be.retry("h3_write", attempt, more)
    return b


def h3_write(hsrc, dsrc, items, item_start, tx):
    """Host arrays: the HTTP/3 frames of many streams written as
    nghttp3_stream_write_header_block and nghttp3_stream_write_data write them.
    items: H3_ITEM_DTYPE records (off, len into hsrc when src is 0, the section
    writer's dst, or into dsrc when src is 1; type; flags H3W_END); item_start
    (uint32, one entry more than streams); tx: H3_TX_DTYPE records
    (``h3_tx``), updated in place.  -> dict: dst (the bytes written), out
    (SPAN_IN_DTYPE, a stream's bytes of this call), fin (uint8), status (int32: 0
    or QH_ERR_INVALID_STATE): out, fin, stream ids and views are the chunks of
    ``h3_read`` on the peer.  Runs on the host (qh_qpack_h3_write)."""
    hsrc, dsrc = _u8(hsrc), _u8(dsrc)
    items = np.ascontiguousarray(items, H3_ITEM_DTYPE)
    start = np.ascontiguousarray(item_start, np.uint32)
    n = start.size - 1
    if n < 0 or tx.dtype != H3_TX_DTYPE or tx.size != n or not tx.flags.c_contiguous or \
            (n and int(start.max()) > items.size):
        raise ValueError("h3_write: item_start has one entry more than streams, inside items; one record per stream")
    be = Backend()
    b = _h3_write(be, hsrc, dsrc, items.view(np.uint8), start.view(np.uint8), n, tx.view(np.uint8), None)
    return {"dst": b["dst"][:b["dst_need"]], "out": b["out"].view(SPAN_IN_DTYPE)[:n], "fin": b["fin"][:n],
            "status": b["status"].view(np.int32)[:n], "tx": tx}


def h3_write_dev(codec: HuffmanBatchCodec, hsrc, dsrc, items, item_start, tx, bufs=None):
    """Device-resident form (qh_h3_write_batch): uint8 tensors holding the same
    records (hsrc, dsrc; items [nitems * 32]; item_start [(n + 1) * 4]; tx
    [n * 16] updated in place).  -> dict of uint8 tensors dst (dst_need bytes
    written), out [n * 16], fin [n], status [n * 4], plus the host integer
    dst_need; `bufs` (a previous result) reuses its allocations.  out and fin
    go as they are into ``h3_read_dev`` with dst as its src.  One host wait,
    for the byte total."""
    n = int(item_start.shape[0]) // 4 - 1
    return _h3_write(Backend(tx.device if n else item_start.device), hsrc, dsrc, items, item_start, n, tx, bufs,
                     codec=codec)


# ---- unidirectional streams as they arrive (qh_qpack_h3_uni_read / qh_h3_uni_read_batch, _settings_apply) ----

def h3_unis(n: int):
    """n fresh H3_UNI_DTYPE records (qh_h3_uni_init): not identified yet."""
    us = np.zeros(n, dtype=H3_UNI_DTYPE)
    if n:
        _load().qh_h3_uni_init(_vp(us), n)
    return us


def h3_conns(n: int, server: bool = True, max_client_streams: int = 0):
    """n fresh H3_CONN_DTYPE records (qh_h3_conn_init): the remote settings,
    goaway_id and flags as nghttp3_conn_new leaves them; `max_client_streams`
    bounds the element id of a PRIORITY_UPDATE."""
    cs = np.zeros(n, dtype=H3_CONN_DTYPE)
    if n:
        _load().qh_h3_conn_init(_vp(cs), n, 1 if server else 0, int(max_client_streams))
    return cs


# The outputs of a read: name -> bytes per chunk; nglitch is per connection.
_H3U_OUT = (("status", 4), ("consumed", 4), ("enc_pieces", 16), ("enc_conn", 4), ("dec_pieces", 16),
            ("dec_conn", 4))


def h3_uni_read_raw(be, src, chunks, chunk_fin, chunk_sid, nchunks, conn_start, nconns, us, cs, o, event_cap,
                    codec=None):
    """The call over byte arrays of backend `be` -> (rv, nenc, ndec, nevents).
    `o`: the outputs of _H3U_OUT plus nglitch and events (either may be None);
    event_cap the room of events in records."""
    ne, nd, nv = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rv = be.call(_load(), "h3_uni_read", be.ptr(src), be.ptr(chunks), be.ptr(chunk_fin), be.ptr(chunk_sid),
                 nchunks, be.ptr(conn_start), nconns, be.ptr(us), be.ptr(cs), be.ptr(o["status"]),
                 be.ptr(o["consumed"]), be.ptr(o.get("nglitch")), be.ptr(o["enc_pieces"]), be.ptr(o["enc_conn"]),
                 ctypes.byref(ne), be.ptr(o["dec_pieces"]), be.ptr(o["dec_conn"]), ctypes.byref(nd),
                 be.ptr(o.get("events")), event_cap, ctypes.byref(nv), codec=codec)
    return rv, int(ne.value), int(nd.value), int(nv.value)


def _h3_uni_read(be, src, chunks, chunk_fin, chunk_sid, n, conn_start, nconns, us, cs, bufs, codec=None):
    b = bufs or {}
    if b.get("n", -1) < n or b.get("nconns", -1) < nconns:
        b = {"n": n, "nconns": nconns, "event_cap": b.get("event_cap", 0), "events": b.get("events")}
        for name, unit in _H3U_OUT:
            b[name] = be.empty(max(n, 1) * unit)
        b["nglitch"] = be.empty(max(nconns, 1) * 4)
    if b["events"] is None:
        b["event_cap"] = cap_for(nconns, 64)
        b["events"] = be.empty(b["event_cap"] * 32)

    def attempt():
        rv, ne, nd, nv = h3_uni_read_raw(be, src, chunks, chunk_fin, chunk_sid, n, conn_start, nconns, us, cs, b,
                                         b["event_cap"], codec=codec)
        return rv, (ne, nd, nv)

    def more(needs):
        b["event_cap"] = cap_for(needs[2], 64)
        b["events"] = be.empty(b["event_cap"] * 32)

    _, (b["nenc"], b["ndec"], b["nevents"]) = be.retry("h3_uni_read", attempt, more)
    return b


def h3_uni_read(src, chunks, chunk_fin, chunk_sid, conn_start, us, cs):
    """Host arrays: the new bytes of the peers' unidirectional streams of many
    connections, read as nghttp3_conn_read_uni reads them.  chunks:
    SPAN_IN_DTYPE spans into src with chunk_fin (uint8) and chunk_sid (uint64);
    conn_start (uint32, one entry more than connections): connection k owns
    chunks [conn_start[k], conn_start[k + 1]) in arrival order; us:
    H3_UNI_DTYPE records (``h3_unis``), one per chunk; cs: H3_CONN_DTYPE
    records (``h3_conns``); both updated in place.  -> dict: status (H3U_OPEN,
    H3U_GONE or the error) and consumed per chunk, nglitch per connection;
    enc_pieces / enc_conn (the QPACK encoder streams' bytes behind the type,
    for ``DynamicTableSet.feed_encoder(src, pieces, tsel)``), dec_pieces /
    dec_conn (the same for ``EncoderSet.feed_decoder``), events
    (H3_EVENT_DTYPE).  Runs on the host (qh_qpack_h3_uni_read)."""
    src = _u8(src)
    chunks = np.ascontiguousarray(chunks, SPAN_IN_DTYPE)
    n = chunks.size
    fin, sid = np.ascontiguousarray(chunk_fin, np.uint8), np.ascontiguousarray(chunk_sid, np.uint64)
    start = np.ascontiguousarray(conn_start, np.uint32)
    nconns = start.size - 1
    if fin.size != n or sid.size != n or us.dtype != H3_UNI_DTYPE or us.size != n or nconns < 0 or \
            cs.dtype != H3_CONN_DTYPE or cs.size != nconns or not us.flags.c_contiguous or \
            not cs.flags.c_contiguous:
        raise ValueError("h3_uni_read: one fin, sid and stream record per chunk, one record per connection")
    be = Backend()
    b = _h3_uni_read(be, src, chunks.view(np.uint8), fin, sid.view(np.uint8), n, start.view(np.uint8), nconns,
                     us.view(np.uint8), cs.view(np.uint8), None)
    ne, nd, nv = b["nenc"], b["ndec"], b["nevents"]
    return {"status": b["status"].view(np.int32)[:n], "consumed": b["consumed"].view(np.uint32)[:n],
            "nglitch": b["nglitch"].view(np.uint32)[:nconns], "nenc": ne, "ndec": nd, "nevents": nv,
            "enc_pieces": b["enc_pieces"].view(SPAN_IN_DTYPE)[:ne], "enc_conn": b["enc_conn"].view(np.uint32)[:ne],
            "dec_pieces": b["dec_pieces"].view(SPAN_IN_DTYPE)[:nd], "dec_conn": b["dec_conn"].view(np.uint32)[:nd],
            "events": b["events"].view(H3_EVENT_DTYPE)[:nv], "us": us, "cs": cs}


def h3_uni_read_dev(codec: HuffmanBatchCodec, src, chunks, chunk_fin, chunk_sid, conn_start, us, cs, bufs=None):
    """Device-resident form (qh_h3_uni_read_batch): uint8 tensors holding the
    same records (chunks [n * 16], chunk_fin [n], chunk_sid [n * 8], conn_start
    [(nconns + 1) * 4], us [n * 32] and cs [nconns * 64] updated in place).  ->
    dict of uint8 tensors named as h3_uni_read's arrays, with room for n chunks
    (the first nenc / ndec / nevents entries are written), plus those three
    host integers; `bufs` (a previous result) reuses its allocations.  One host
    wait, for the three totals."""
    n = int(chunk_fin.shape[0])
    nconns = int(conn_start.shape[0]) // 4 - 1
    return _h3_uni_read(Backend(conn_start.device), src, chunks, chunk_fin, chunk_sid, n, conn_start, nconns, us,
                        cs, bufs, codec=codec)


def h3_settings_apply(cs, acct, enc, csel=None):
    """Host arrays: the peer's SETTINGS of the listed connections (csel uint32;
    None: all) put to their encoders, in place (qh_qpack_h3_settings_apply):
    cs H3_CONN_DTYPE, acct ACCT_DTYPE, enc ENC_STATE_DTYPE, one per
    connection."""
    n = cs.size
    if cs.dtype != H3_CONN_DTYPE or acct.dtype != ACCT_DTYPE or enc.dtype != ENC_STATE_DTYPE or \
            acct.size != n or enc.size != n:
        raise ValueError("h3_settings_apply: one acct and enc record per connection record")
    sel = _as(csel, np.uint32)
    be = Backend()
    rv = be.call(_load(), "h3_settings_apply", be.ptr(cs.view(np.uint8)), be.list_ptr(sel),
                 0 if sel is None else sel.size, n, be.ptr(acct.view(np.uint8)), be.ptr(enc.view(np.uint8)))
    be.check(rv, "h3_settings_apply")


def h3_settings_apply_dev(codec: HuffmanBatchCodec, cs, acct, enc, csel=None):
    """Device-resident form (qh_h3_settings_apply_batch): uint8 tensors cs
    [n * 64], acct [n * 32], enc [n * 64] updated in place, csel int32 / uint32
    indices or None.  Asynchronous on the context's stream: no host wait."""
    n = int(cs.shape[0]) // H3_CONN_DTYPE.itemsize
    be = Backend(cs.device)
    rv = be.call(_load(), "h3_settings_apply", be.ptr(cs), be.list_ptr(csel),
                 0 if csel is None else int(csel.shape[0]), n, be.ptr(acct), be.ptr(enc), codec=codec)
    be.check(rv, "h3_settings_apply")


def h3_write_settings(max_field_section_size: int = (1 << 62) - 1, qpack_max_dtable_capacity: int = 0,
                      qpack_blocked_streams: int = 0, enable_connect_protocol: bool = False,
                      h3_datagram: bool = False) -> bytes:
    """The opening bytes of this side's control stream (qh_h3_write_settings):
    the stream type and the SETTINGS frame as nghttp3_stream_write_stream_type
    and nghttp3_stream_write_settings write them."""
    s = np.zeros(1, H3_SETTINGS_DTYPE)
    s["max_field_section_size"], s["qpack_max_dtable_capacity"] = max_field_section_size, qpack_max_dtable_capacity
    s["qpack_blocked_streams"] = qpack_blocked_streams
    s["enable_connect_protocol"], s["h3_datagram"] = bool(enable_connect_protocol), bool(h3_datagram)
    lib = _load()
    n = lib.qh_h3_write_settings(None, _vp(s))
    buf = np.zeros(n, np.uint8)
    assert lib.qh_h3_write_settings(_vp(buf), _vp(s)) == n
    return buf.tobytes()


# ---- streams by id (qh_qpack_h3_dispatch / qh_h3_dispatch_batch, _commit, _open, _find, _recs_move, _close, _shutdown) ----

class H3Smaps:
    """The stream tables of n connections (include/qhuff.h "Streams by id"):
    the connection records ``sm`` (H3_SMAP_DTYPE), the slot, entry
    (H3_SENT_DTYPE) and gap (H3_GAP_DTYPE) arrays and the per-stream pools
    ``rs_pool`` (H3_STREAM_DTYPE), ``hs_pool`` (HTTP_STATE_DTYPE) and ``us_pool``
    (H3_UNI_DTYPE), all as bytes on one backend: numpy arrays, or uint8 tensors
    on `device`.  ``h3_smaps`` makes one; the h3_* functions below work on it."""

    def __init__(self, n: int, rec_cap, server: bool = True, device=None, codec=None):
        caps = np.ascontiguousarray(np.broadcast_to(np.asarray(rec_cap, np.uint32), (n,)))
        sm = np.zeros(n, dtype=H3_SMAP_DTYPE)
        tot = np.zeros(3, np.uint64)
        _lib.check(_load().qh_h3_smap_init(_vp(sm), n, 1 if server else 0, _vp(caps), _vp(tot)), "qh_h3_smap_init")
        be = self.be = Backend(device, codec)
        self.n, self.server = n, bool(server)
        self.nslots, self.nrecs, self.ngaps = (int(x) for x in tot)
        self.sm = be.put(sm.view(np.uint8))
        self.slots, self.gaps = be.zeros(self.nslots * 4), be.zeros(self.ngaps * 16)
        self.ents, self.rs_pool = be.zeros(self.nrecs * 32), be.zeros(self.nrecs * 32)
        self.hs_pool, self.us_pool = be.zeros(self.nrecs * 16), be.zeros(self.nrecs * 32)

    ARRAYS = ("sm", "slots", "ents", "gaps", "rs_pool", "hs_pool", "us_pool")
    _DTYPES = {"sm": H3_SMAP_DTYPE, "slots": np.uint32, "ents": H3_SENT_DTYPE, "gaps": H3_GAP_DTYPE,
               "rs_pool": H3_STREAM_DTYPE, "hs_pool": HTTP_STATE_DTYPE, "us_pool": H3_UNI_DTYPE}

    def tab(self):
        p = self.be.ptr
        return qh_h3d_tab(p(self.sm), self.n, p(self.slots), self.nslots, p(self.ents), self.nrecs, p(self.gaps),
                          self.ngaps, p(self.rs_pool), p(self.hs_pool), p(self.us_pool))

    def records(self, name: str):
        """A typed numpy copy of one of ARRAYS."""
        return self.be.host(getattr(self, name)).view(self._DTYPES[name])

    def load(self, other: "H3Smaps"):
        """The state of `other` (the same layout, any backend) copied into this one."""
        for name in self.ARRAYS:
            setattr(self, name, self.be.put(other.be.host(getattr(other, name))))
        return self

    def _b(self, a, dtype):
        if isinstance(a, np.ndarray) or not self.be.dev:
            a = np.ascontiguousarray(a, dtype).reshape(-1).view(np.uint8)
            return self.be.put(a) if self.be.dev else a
        return a


def h3_smaps(n: int, rec_cap, server: bool = True, device=None, codec=None) -> H3Smaps:
    """The stream tables of n connections with room for rec_cap (one number or
    one per connection) live streams each; `device`: in HBM."""
    return H3Smaps(n, rec_cap, server=server, device=device, codec=codec)


def h3_dispatch(maps: H3Smaps, stream_id, chunks, fin, conn_start, out=None, codec=None):
    """The arrivals of one call routed to their streams' records
    (nghttp3_conn_read_stream2 up to its last two lines).  stream_id (uint64),
    chunks (SPAN_IN_DTYPE) and fin (uint8) per arrival, conn_start (uint32, one
    entry more than connections); numpy arrays, or uint8 tensors for tables in
    HBM.  -> dict of byte arrays of the tables' backend: route (int32) and rec
    (uint32) per arrival and the lists of H3D_LISTS with room for every
    arrival, plus the host integers n, nbidi, nuni and rv.  `out` (arrays by
    those names): written in place of fresh ones, and rv is handed back
    unchecked.  One host wait on the device."""
    be = maps.be
    sid, ch, fn = maps._b(stream_id, np.uint64), maps._b(chunks, SPAN_IN_DTYPE), maps._b(fin, np.uint8)
    start = maps._b(conn_start, np.uint32)
    n = int(fn.shape[0])
    o = dict(out) if out is not None else {}
    for name, unit in (("route", 4), ("rec", 4)) + H3D_LISTS:
        if name not in o:
            o[name] = be.empty((maps.n + 1 if name == "u_conn_start" else max(n, 1)) * unit)
    lists = qh_h3d_lists(*[be.ptr(o[name]) for name, _ in H3D_LISTS])
    nb, nu = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rv = be.call(_load(), "h3_dispatch", ctypes.byref(maps.tab()), be.ptr(sid), be.ptr(ch), be.ptr(fn), n,
                 be.ptr(start), be.ptr(o["route"]), be.ptr(o["rec"]), ctypes.byref(lists), ctypes.byref(nb),
                 ctypes.byref(nu), codec=codec)
    if out is None:
        be.check(rv, "h3_dispatch")
    o.update(n=n, nbidi=int(nb.value), nuni=int(nu.value), rv=rv)
    return o


def h3_dispatch_dev(codec: HuffmanBatchCodec, maps: H3Smaps, stream_id, chunks, fin, conn_start, out=None):
    """Device-resident form (qh_h3_dispatch_batch) of ``h3_dispatch``."""
    return h3_dispatch(maps, stream_id, chunks, fin, conn_start, out=out, codec=codec)


def h3_commit(maps: H3Smaps, d, codec=None) -> int:
    """The records of a dispatch `d` (its b_rec, rs_call, hs_call, u_rec,
    us_call as the round's calls left them) scattered back into the pools;
    -> the entries passed over (host), or a one-word tensor holding that count
    (device: no host wait)."""
    be = maps.be
    skipped = be.zeros(4)
    rv = be.call(_load(), "h3_commit", ctypes.byref(maps.tab()), be.ptr(d["b_rec"]), be.ptr(d["rs_call"]),
                 be.ptr(d["hs_call"]), d["nbidi"], be.ptr(d["u_rec"]), be.ptr(d["us_call"]), d["nuni"],
                 be.ptr(skipped), codec=codec)
    be.check(rv, "h3_commit")
    return skipped if be.dev else int(skipped.view(np.uint32)[0])


def h3_commit_dev(codec: HuffmanBatchCodec, maps: H3Smaps, d):
    return h3_commit(maps, d, codec=codec)


def _h3_items(maps, stream_id, conn_start):
    sid, start = maps._b(stream_id, np.uint64), maps._b(conn_start, np.uint32)
    return sid, start, int(sid.shape[0]) // 8


def h3_open(maps: H3Smaps, cs, stream_id, conn_start, codec=None, checked=True):
    """A client's own request streams created (the create half of
    nghttp3_conn_submit_request): ids grouped per connection by conn_start, cs
    the H3_CONN_DTYPE records.  -> (status int32 bytes, rec uint32 bytes, rv)."""
    be = maps.be
    sid, start, n = _h3_items(maps, stream_id, conn_start)
    status, rec = be.empty(max(n, 1) * 4), be.empty(max(n, 1) * 4)
    conns = maps._b(cs, H3_CONN_DTYPE)
    rv = be.call(_load(), "h3_open", ctypes.byref(maps.tab()), be.ptr(conns), be.ptr(sid), n,
                 be.ptr(start), be.ptr(status), be.ptr(rec), codec=codec)
    if checked:
        be.check(rv, "h3_open")
    return status[:n * 4], rec[:n * 4], rv


def h3_open_dev(codec: HuffmanBatchCodec, maps: H3Smaps, cs, stream_id, conn_start, checked=True):
    return h3_open(maps, cs, stream_id, conn_start, codec=codec, checked=checked)


def h3_find(maps: H3Smaps, conn, stream_id, codec=None):
    """rec (uint32 bytes) for each (conn, stream_id), H3D_NOREC when the stream
    is not in the table.  No host wait on the device."""
    be = maps.be
    cn, sid = maps._b(conn, np.uint32), maps._b(stream_id, np.uint64)
    n = int(cn.shape[0]) // 4
    rec = be.empty(max(n, 1) * 4)
    rv = be.call(_load(), "h3_find", ctypes.byref(maps.tab()), be.ptr(cn), be.ptr(sid), n, be.ptr(rec), codec=codec)
    be.check(rv, "h3_find")
    return rec[:n * 4]


def h3_find_dev(codec: HuffmanBatchCodec, maps: H3Smaps, conn, stream_id):
    return h3_find(maps, conn, stream_id, codec=codec)


def h3_recs_move(be: Backend, pool, call, idx, rec_bytes: int, scatter: bool, codec=None):
    """Records of 16, 32 or 64 bytes gathered from `pool` into `call` at
    idx[j] (uint32 bytes), or scattered back (byte arrays of backend `be`):
    how a pool the caller keeps beside the tables (H3_TX_DTYPE) is moved."""
    n = int(idx.shape[0]) // 4
    rv = be.call(_load(), "h3_recs_move", be.ptr(pool), int(pool.shape[0]) // rec_bytes, be.ptr(call), be.ptr(idx),
                 n, rec_bytes, 1 if scatter else 0, codec=codec)
    be.check(rv, "h3_recs_move")


def h3_close(maps: H3Smaps, stream_id, conn_start, codec=None, checked=True):
    """Streams closed (nghttp3_conn_close_stream2), ids grouped per connection
    by conn_start.  -> dict: status (int32 bytes), cancel_sid / cancel_view
    (the closed bidi streams, for ``cancel`` of the blocked and partial
    queues), drained (uint8 per connection), the host integers ncancel, rv."""
    be = maps.be
    sid, start, n = _h3_items(maps, stream_id, conn_start)
    o = {"status": be.empty(max(n, 1) * 4), "cancel_sid": be.empty(max(n, 1) * 8),
         "cancel_view": be.empty(max(n, 1) * 4), "drained": be.empty(max(maps.n, 1))}
    nc = ctypes.c_uint64(0)
    rv = be.call(_load(), "h3_close", ctypes.byref(maps.tab()), be.ptr(sid), n, be.ptr(start), be.ptr(o["status"]),
                 be.ptr(o["cancel_sid"]), be.ptr(o["cancel_view"]), ctypes.byref(nc), be.ptr(o["drained"]),
                 codec=codec)
    if checked:
        be.check(rv, "h3_close")
    o.update(n=n, ncancel=int(nc.value), rv=rv)
    return o


def h3_close_dev(codec: HuffmanBatchCodec, maps: H3Smaps, stream_id, conn_start, checked=True):
    return h3_close(maps, stream_id, conn_start, codec=codec, checked=checked)


def h3_shutdown(maps: H3Smaps, kind: int = H3D_SHUTDOWN, csel=None, codec=None, checked=True):
    """nghttp3_conn_shutdown (H3D_SHUTDOWN) or _submit_shutdown_notice
    (H3D_NOTICE) for the listed connections (uint32; None: all).  ->
    (goaway_id uint64 bytes, status int32 bytes, rv): the ids to frame."""
    be = maps.be
    sel = None if csel is None else maps._b(csel, np.uint32)
    n = maps.n if sel is None else int(sel.shape[0]) // 4
    ids, status = be.empty(max(n, 1) * 8), be.empty(max(n, 1) * 4)
    rv = be.call(_load(), "h3_shutdown", ctypes.byref(maps.tab()), be.list_ptr(sel), n, kind, be.ptr(ids),
                 be.ptr(status), codec=codec)
    if checked:
        be.check(rv, "h3_shutdown")
    return ids[:n * 8], status[:n * 4], rv


def h3_shutdown_dev(codec: HuffmanBatchCodec, maps: H3Smaps, kind: int = H3D_SHUTDOWN, csel=None, checked=True):
    return h3_shutdown(maps, kind, csel, codec=codec, checked=checked)


class DynamicTable:
    """The decoder's dynamic table (qh_dtable_*): ``apply`` feeds it
    encoder-stream bytes, ``view`` is its current state (one VIEW_DTYPE
    record; it stays valid after later applies, the log being append-only),
    ``entries`` / ``bytes`` the log, ``to_device`` its copy in HBM."""

    def __init__(self, hard_max: int):
        self._lib = _load()
        h = ctypes.c_void_p()
        _lib.check(self._lib.qh_dtable_new(ctypes.byref(h), hard_max), "qh_dtable_new")
        self._h = h
        self._dev = None  # to_device's tensors and how much of the log they hold

    def close(self):
        if self._h:
            self._lib.qh_dtable_del(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, record_bytes) -> int:
        """Scans the encoder-stream bytes, decodes their Huffman strings (the
        scalar drop-in) and applies the complete instructions.  Returns the
        bytes consumed (a trailing partial instruction is left to the
        caller); raises QhError with the reference's error (-402, -109)."""
        from .qpack_huffman import HuffmanDecodeContext, huffman_decode, huffman_decode_context_init
        buf = _u8(record_bytes)
        rv, insts, spans = scan_encoder_stream(buf)
        _lib.check(rv, "qh_qpack_scan_encoder_stream")
        strs = np.zeros(max(spans.size, 1), dtype=SPAN_OUT_DTYPE)
        dec = bytearray()
        for k, s in enumerate(spans):
            if s["flags"] & SPAN_HUFFMAN:
                ctx = HuffmanDecodeContext()
                huffman_decode_context_init(ctx)
                out = huffman_decode(ctx, buf[int(s["off"]):int(s["off"]) + int(s["len"])], True)
                if isinstance(out, int):
                    raise _lib.QhError(QH_ERR_QPACK_ENCODER_STREAM_ERROR, "encoder stream Huffman string")
                strs[k] = (len(dec), len(out), 0)
                dec += out
        d = _u8(bytes(dec))
        insts = np.ascontiguousarray(insts)
        spans = np.ascontiguousarray(spans)
        _lib.check(self._lib.qh_dtable_apply(self._h, _vp(insts), insts.size, _vp(buf), _vp(spans),
                                             _vp(d), _vp(strs)), "qh_dtable_apply")
        return int(rv)

    def view(self):
        v = np.zeros(1, dtype=VIEW_DTYPE)
        _lib.check(self._lib.qh_dtable_get_view(self._h, _vp(v)), "qh_dtable_get_view")
        return v

    def _log(self, fn, dtype):
        n = ctypes.c_size_t(0)
        p = fn(self._h, ctypes.byref(n))
        if not n.value:
            return np.zeros(0, dtype=dtype)
        nbytes = n.value * np.dtype(dtype).itemsize
        return np.frombuffer(ctypes.string_at(p, nbytes), dtype=dtype)

    def entries(self):
        """A copy of the entry log (DYN_ENTRY_DTYPE; entry a is record a)."""
        return self._log(self._lib.qh_dtable_entries, DYN_ENTRY_DTYPE)

    def bytes(self):
        """A copy of the byte log."""
        return self._log(self._lib.qh_dtable_bytes, np.uint8)

    def keys(self):
        """The entry log's keys (DYN_KEY_DTYPE, qh_qpack_dyn_keys): kept, and
        only the tail appended since the last call is computed."""
        ents, byts = self.entries(), self.bytes()
        have = getattr(self, "_keys", None)
        if have is None:
            have = np.zeros(0, dtype=DYN_KEY_DTYPE)
        if ents.size > have.size:
            have = dyn_keys(ents, byts, first=have.size, keys=have)
        self._keys = have
        return have

    def index(self, rebuild=False, max_buckets=0):
        """The hashed index over the current view's keys (dyn_index): built at
        the first call and kept; only ``rebuild=True`` builds it again.  The
        log never relocates, so an older index stays usable after later
        applies: the planners scan the entries inserted since and walk the
        chains for the rest."""
        if rebuild or getattr(self, "_index", None) is None:
            self._index = dyn_index(self.view(), self.keys(), max_buckets=max_buckets)
        return self._index

    def to_device(self, device):
        """-> {"views" uint8 [40], "entries" uint8 [n * 32], "bytes" uint8,
        "keys" uint8 [n * 16], "nentries", "nbytes", "index"} torch tensors
        on `device` holding the current state, the log and its keys.  Only the
        records, keys and bytes appended since the last upload are copied
        (the tensors are kept, with room to grow).  "index": the tensors of
        the index ``index()`` keeps ({"recs" uint8 [48], "slots" uint8,
        "nslots"}), uploaded once per build; None when none was built."""
        import torch
        ents, byts, keys = self.entries(), self.bytes(), self.keys()
        d = self._dev
        if d is None or d["device"] != torch.device(device):
            d = self._dev = {"device": torch.device(device), "ne": 0, "nb": 0, "nk": 0,
                             "entries": torch.empty(0, dtype=torch.uint8, device=device),
                             "bytes": torch.empty(0, dtype=torch.uint8, device=device),
                             "keys": torch.empty(0, dtype=torch.uint8, device=device)}
        for key, have, host in (("entries", "ne", ents.view(np.uint8)), ("bytes", "nb", byts),
                                ("keys", "nk", keys.view(np.uint8))):
            if host.size > d[key].numel():  # grow: keep what is there
                t = torch.empty(max(2 * host.size, 4096), dtype=torch.uint8, device=device)
                t[:d[have]] = d[key][:d[have]]
                d[key] = t
            if host.size > d[have]:
                d[key][d[have]:host.size] = torch.from_numpy(host[d[have]:].copy()).to(device)
                d[have] = host.size
        views = torch.from_numpy(self.view().view(np.uint8).copy()).to(device)
        ix = getattr(self, "_index", None)
        if ix is None:
            d["index"] = d["index_of"] = None
        elif d.get("index_of") is not ix:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)
            d["index"] = {"recs": up(ix["recs"]), "slots": up(ix["slots"]), "nslots": ix["nslots"]}
            d["index_of"] = ix
        return {"views": views, "entries": d["entries"], "bytes": d["bytes"], "keys": d["keys"],
                "nentries": int(ents.size), "nbytes": int(byts.size), "index": d["index"]}


class HeldStreams:
    """The encoder or decoder streams of `n` tables or connections as they
    arrive (qh_ustream_* / qh_qpack_ustream_*): one USTREAM_DTYPE record each
    in ``us`` (uint8 [n * 32]) and the append-only byte log ``log`` /
    ``nlog`` that holds every joined stream, the cut instructions among them.
    `be` is the owning state object's Backend; a device form without a codec
    of its own takes one per call."""

    def __init__(self, lib, be, n: int):
        self._lib, self._be, self.n = lib, be, int(n)
        # (a fresh record is all zeros: qh_ustream_init)
        self.us = be.put(np.zeros(self.n * 32, dtype=np.uint8))
        self.log = be.empty(4096)
        self.nlog = 0

    _grow = grow

    def join(self, src, pieces, tsel, limit, codec=None, cap=None):
        """-> (rv, need, joined, verdict): joined the listed streams' spans of
        ``log`` (bytes, 16 per stream), ready to be `streams` with src =
        ``log``; verdict int32; need the log's length after the call (on
        QH_ERR_NOMEM: what it would be).  cap: a fixed capacity of the log
        instead of growing, as the other state calls take ``caps=``; rv is
        then the call's return value, unchecked."""
        be = self._be
        ptr = be.ptr
        nsel = self.n if tsel is None else be.size(tsel)
        # (a call that returns 0 writes every listed entry of both)
        joined = be.empty(max(nsel, 1) * 16)
        verdict = be.empty(max(nsel, 1), np.int32)
        fixed = cap is not None

        def attempt():
            n = ctypes.c_uint64(self.nlog)
            rv = be.call(self._lib, "ustream_join", ptr(src), ptr(pieces), be.list_ptr(tsel), nsel, self.n,
                         limit, ptr(self.us), ptr(self.log), ctypes.byref(n),
                         cap if fixed else be.size(self.log), ptr(joined), ptr(verdict), codec=codec)
            return rv, int(n.value)
        rv, need = be.retry("ustream_join", attempt, lambda need: self._grow("log", self.nlog, need, 4096),
                            fixed)
        if rv == 0:
            self.nlog = need
        return rv, need, joined[:nsel * 16], verdict[:nsel]

    def keep(self, status, consumed, tsel, opts, codec=None, check=True):
        be = self._be
        nsel = self.n if tsel is None else be.size(tsel)
        rv = be.call(self._lib, "ustream_keep", be.ptr(status), be.ptr(consumed), be.list_ptr(tsel), nsel,
                     self.n, opts, be.ptr(self.us), codec=codec)
        if check:
            be.check(rv, "ustream_keep")
        return rv

    def sections(self, status, block_view, codec=None, check=True):
        be = self._be
        # (an emit result's status may have room behind its blocks: the list says how many there are)
        nblocks = be.size(status) if block_view is None else be.size(block_view)
        assert nblocks <= be.size(status)
        rv = be.call(self._lib, "ustream_sections", be.ptr(status), be.list_ptr(block_view), nblocks,
                     self.n, be.ptr(self.us), codec=codec)
        if check:
            be.check(rv, "ustream_sections")
        return rv

    def compact(self, codec=None):
        """Replaces ``log`` by one that holds the tails alone, back to back in
        table order, ``us`` rebased.  A failed call leaves the object as it
        was."""
        be = self._be
        us = be.own(self.us)

        def call(outs):
            n = ctypes.c_uint64(0)
            rv = be.call(self._lib, "ustream_compact", self.n, be.ptr(us), be.ptr(self.log), self.nlog,
                         be.ptr(outs[0]), ctypes.byref(n), be.size(outs[0]), codec=codec)
            return rv, (int(n.value),)
        (log,), (n,) = be.sized("ustream_compact", call, ((1, 4096),), be.zeros)
        self.us, self.log, self.nlog = us, log, n

    def records(self):
        """-> (us USTREAM_DTYPE [n], log uint8 [nlog]), numpy copies."""
        h = self._be.host
        return h(self.us).view(USTREAM_DTYPE), h(self.log[:self.nlog])

    def feed(self, read, src, pieces, tsel, limit, opts, codec=None):
        """join -> read(log, joined, tsel) -> (status, consumed) -> keep.
        -> status: the join's verdict where that is negative, else the
        read's."""
        _, _, joined, verdict = self.join(src, pieces, tsel, limit, codec)
        status, consumed = read(self.log, joined, tsel)
        self.keep(status, consumed, tsel, opts, codec)
        if self._be.dev:
            return self._be.torch.where(verdict < 0, verdict, status)
        return np.where(verdict < 0, verdict, status)


class DynamicTableSet:
    """The dynamic tables of many connections over one log
    (qh_dtables_apply_batch / qh_qpack_dtables_apply): `ntables` fresh tables
    of hard maximum capacity `hard_max` (a scalar, or one value per table).

    With a `codec` the views, acct records, the log and its keys are torch
    tensors on the codec's device and ``read_encoder_dev`` applies encoder
    streams there; ``views`` (uint8 [ntables * 40]), ``entries`` (uint8),
    ``dyn_bytes`` (uint8), ``nentries`` and ``nbytes`` go straight into
    ``emit_fields_dev(views=, entries=, dyn_bytes=, block_view=)`` and the
    dynamic planners, ``keys()`` with them.  Without a codec the same state is
    numpy arrays and ``read_encoder`` the host twin.  Applying only grows the
    log: a copy of ``views`` taken before a call stays valid after it.
    ``compact()`` replaces the log by one that holds the live records alone.

    With `max_blocked` (a scalar, or one value per table) the set also keeps
    the sections that emit found blocked: ``bq`` (uint8 [ntables * 32],
    DEC_BLKS_DTYPE), the record log ``blks`` / ``nblks`` (DEC_BLK_DTYPE) and
    the byte log ``pend`` / ``npend``, fed by ``push_blocked`` after an emit,
    drained by ``release_blocked`` after ``read_encoder`` and by
    ``cancel_blocked``; ``compact_blocked`` replaces the two logs.

    With `max_section_bytes` (a scalar, or one value per table; the
    project's own limit on a section's length) the set also keeps the
    sections that arrive in pieces until their last piece: ``pq`` (uint8
    [ntables * 32], DEC_PARTS_DTYPE), the record log ``parts`` / ``nparts``
    (DEC_PART_DTYPE) and the byte log ``held`` / ``nheld``, fed by
    ``push_pieces``, which hands the finished sections on whole;
    ``cancel_pieces`` drops the streams that were reset, ``compact_pieces``
    replaces the two logs.  Every continued section leaves its previous copy
    dead in ``held``: this log wants compacting more often than the blocked
    one.

    With ``streams=True`` the set also keeps each table's encoder stream as it
    arrives (``ustreams``, a HeldStreams): ``feed_encoder`` takes whatever
    bytes have come, holds a cut instruction until the rest follows, and
    keeps the reference's sticky failure and its 128 KiB rule;
    ``note_sections`` tells it what an emit call found, ``compact_streams``
    replaces its log, ``stream_records`` reads it back.  ``read_encoder`` is
    unchanged."""

    def __init__(self, hard_max, ntables: int, codec: HuffmanBatchCodec | None = None,
                 max_blocked=None, max_section_bytes=None, streams: bool = False):
        self._lib = _load()
        self.codec = codec
        self.ntables = int(ntables)
        if codec is None:
            be = self._be = Backend()
        else:
            be = self._be = Backend("cuda:%d" % codec.device if hasattr(codec, "device") else "cuda",
                                    codec)
        hm = np.broadcast_to(np.asarray(hard_max, dtype=np.uint64), (self.ntables,))
        views = np.zeros(max(self.ntables, 1), dtype=VIEW_DTYPE)[:self.ntables]
        acct = np.zeros(max(self.ntables, 1), dtype=ACCT_DTYPE)[:self.ntables]
        v1, a1 = np.zeros(1, dtype=VIEW_DTYPE), np.zeros(1, dtype=ACCT_DTYPE)
        for t in range(self.ntables):
            self._lib.qh_dtable_state_init(int(hm[t]), _vp(v1), _vp(a1))
            views[t], acct[t] = v1[0], a1[0]
        self.nentries = 0
        self.nbytes = 0
        self._nkeys = 0
        self.views, self.acct = be.put(views.view(np.uint8).copy()), be.put(acct.view(np.uint8).copy())
        self.entries, self.dyn_bytes, self._keys = be.empty(0), be.empty(0), be.empty(0)
        self.max_blocked = max_blocked
        if max_blocked is not None:
            mb = np.broadcast_to(np.asarray(max_blocked, dtype=np.uint64), (self.ntables,))
            bq = np.zeros(max(self.ntables, 1), dtype=DEC_BLKS_DTYPE)[:self.ntables]
            b1 = np.zeros(1, dtype=DEC_BLKS_DTYPE)
            for t in range(self.ntables):
                self._lib.qh_dec_blks_init(int(mb[t]), _vp(b1))
                bq[t] = b1[0]
            self.nblks = 0
            self.npend = 0
            self.bq = be.put(bq.view(np.uint8).copy())
            self.blks, self.pend = be.empty(0), be.empty(0)
        self.max_section_bytes = max_section_bytes
        if max_section_bytes is not None:
            mx = np.broadcast_to(np.asarray(max_section_bytes, dtype=np.uint64), (self.ntables,))
            pq = np.zeros(max(self.ntables, 1), dtype=DEC_PARTS_DTYPE)[:self.ntables]
            p1 = np.zeros(1, dtype=DEC_PARTS_DTYPE)
            for t in range(self.ntables):
                self._lib.qh_dec_parts_init(int(mx[t]), _vp(p1))
                pq[t] = p1[0]
            self.nparts = 0
            self.nheld = 0
            self.pq = be.put(pq.view(np.uint8).copy())
            self.parts, self.held = be.empty(0), be.empty(0)
        self.ustreams = HeldStreams(self._lib, be, self.ntables) if streams else None

    # -- capacity: the arrays grow by cap_for, the log's prefix kept

    _grow = grow

    def _reserve(self, nentries: int, nbytes: int):
        self._grow("entries", self.nentries * 32, nentries * 32, 4096)
        self._grow("dyn_bytes", self.nbytes, nbytes, 4096)

    def _read_encoder(self, src, streams, tsel):
        be = self._be
        ptr = be.ptr
        nsel = self.ntables if tsel is None else be.size(tsel)
        status = be.empty(max(nsel, 1), np.int32)
        consumed = be.empty(max(nsel, 1), np.int32)

        def attempt():
            ne, nb = ctypes.c_uint64(self.nentries), ctypes.c_uint64(self.nbytes)
            rv = be.call(self._lib, "dtables_apply", ptr(src), ptr(streams), be.list_ptr(tsel), nsel,
                         self.ntables, ptr(self.views), ptr(self.acct), ptr(self.entries),
                         ctypes.byref(ne), be.size(self.entries) // 32, ptr(self.dyn_bytes),
                         ctypes.byref(nb), be.size(self.dyn_bytes), ptr(status), ptr(consumed))
            return rv, (int(ne.value), int(nb.value))
        _, (self.nentries, self.nbytes) = be.retry("dtables_apply", attempt,
                                                   lambda needs: self._reserve(*needs))
        return status[:nsel], consumed[:nsel]

    def read_encoder_dev(self, src, streams, tsel=None):
        """Applies encoder-stream bytes on the device: stream p is
        src[streams[p, 0], + streams[p, 1] & 0xFFFFFFFF) (torch tensors in
        HBM: src uint8, streams int64 [nsel, 2] as SPAN_IN_DTYPE records,
        tsel int32 [nsel] or None for stream p -> table p).  -> (status int32
        [nsel], consumed int32 [nsel]) tensors: per stream 0 or the first
        failing instruction's error (-402, -109), and the bytes of complete,
        applied instructions.  Asynchronous on the codec stream after the
        call's host waits."""
        assert self.codec is not None
        return self._read_encoder(src, streams, tsel)

    def read_encoder(self, src, streams, tsel=None):
        """The host twin (qh_qpack_dtables_apply) over numpy arrays: src
        uint8, streams SPAN_IN_DTYPE, tsel uint32 or None.  -> (status int32,
        consumed uint32)."""
        assert self.codec is None
        status, consumed = self._read_encoder(_u8(src), _as(streams, SPAN_IN_DTYPE),
                                              _as(tsel, np.uint32))
        return status, consumed.view(np.uint32)

    # -- the encoder streams as they arrive (streams=True): qh_ustream_* / qh_qpack_ustream_*

    def _ustreams(self):
        if self.ustreams is None:
            raise ValueError("the set was made without streams=True")
        return self.ustreams

    def feed_encoder(self, src, pieces, tsel=None):
        """Encoder-stream bytes as they arrive (host form): piece p is
        src[pieces[p].off, + len) (SPAN_IN_DTYPE), the new bytes of table
        tsel[p]'s stream (None: table p), cut anywhere.  Runs join -> apply
        (growing the table log as ``read_encoder`` does) -> keep.  -> status
        int32 per piece: 0, the first failing instruction's error (reported
        with the piece that completes the instruction), -402 once more than
        128 KiB have come without a finished section, -108 for every piece
        after a failure."""
        assert self.codec is None
        return self._ustreams().feed(self._read_encoder, _u8(src), _as(pieces, SPAN_IN_DTYPE),
                                     _as(tsel, np.uint32), USTREAM_MAX_ENCODERLEN, USTREAM_LATCH)

    def feed_encoder_dev(self, src, pieces, tsel=None):
        """The same over torch tensors in HBM (src uint8, pieces int64 [nsel, 2]
        as SPAN_IN_DTYPE records, tsel int32 or None): qh_ustream_join_batch,
        qh_dtables_apply_batch, qh_ustream_keep_batch.  -> status int32
        tensor.  One host wait more than ``read_encoder_dev``, for the join's
        total."""
        assert self.codec is not None
        return self._ustreams().feed(self._read_encoder, src, pieces, tsel, USTREAM_MAX_ENCODERLEN,
                                     USTREAM_LATCH)

    def note_sections(self, emit_result, block_view):
        """After an emit call: a table with a section that finished may take
        another 128 KiB of encoder stream, a table with one that failed reads
        no more (arrays of the object's kind: the result's status, block_view
        uint32 / int32 or None for table 0)."""
        st = self._ustreams()
        if self.codec is None:
            return st.sections(_as(emit_result["status"], np.int32), _as(block_view, np.uint32))
        return st.sections(emit_result["status"], block_view)

    def compact_streams(self):
        """Replaces the streams' log by one that holds the cut instructions
        alone.  When to call is the caller's decision; after every
        ``feed_encoder`` it costs the tails alone."""
        self._ustreams().compact()

    def stream_records(self):
        """-> (us USTREAM_DTYPE [ntables], log uint8 [nlog]), numpy copies."""
        return self._ustreams().records()

    def _write_decoder(self, emit_result, block_sid, block_view, cancel, dst_cap):
        be = self._be
        ptr = be.ptr
        if getattr(self, "written_icnt", None) is None:
            self.written_icnt = be.zeros(max(self.ntables, 1) * 8)
        csid, cview = (None, None) if cancel is None else cancel
        dstreams = be.zeros(max(self.ntables, 1) * 16)
        fixed = dst_cap is not None
        cap, dst = dst_cap if fixed else getattr(self, "_wd_cap", 256), None

        def attempt():
            nonlocal dst
            dst = be.room(cap, 64 if fixed else 0)  # (tests: sentinel bytes behind a fixed capacity)
            need = ctypes.c_uint64(0)
            rv = be.call(self._lib, "dec_write_decoder", ptr(block_sid), ptr(block_view),
                         ptr(emit_result["status"]), ptr(emit_result["ricnt"]), be.size(block_sid),
                         ptr(csid), ptr(cview), be.size(csid), ptr(self.views), self.ntables,
                         ptr(self.written_icnt), ptr(dst), cap, ptr(dstreams), ctypes.byref(need))
            return rv, int(need.value)

        def enlarge(need):
            nonlocal cap
            cap = self._wd_cap = cap_for(need, cap)
        rv, need = be.retry("dec_write_decoder", attempt, enlarge, fixed)
        return {"rv": rv, "dst": dst, "dstreams": dstreams[:self.ntables * 16], "dst_need": need}

    def write_decoder(self, emit_result, block_sid, block_view, cancel=None, dst_cap=None):
        """The decoder streams after an ``emit_fields`` call (host form,
        qh_qpack_dec_write_decoder): block_sid uint64 and block_view uint32,
        one per emitted block (a table's blocks consecutive), cancel =
        (stream ids uint64, tables uint32) or None.  -> dict: dst (uint8),
        dstreams (SPAN_IN_DTYPE, one span per table: its Section
        Acknowledgments, Stream Cancellations and Insert Count Increment),
        dst_need, rv.  The object owns ``written_icnt`` (uint64 per table).
        dst_cap: a fixed capacity instead of growing (the call's return value
        is then handed back in ``rv``)."""
        assert self.codec is None
        er = {"status": _as(emit_result["status"], np.int32), "ricnt": _as(emit_result["ricnt"], np.uint64)}
        c = None if cancel is None else (_as(cancel[0], np.uint64), _as(cancel[1], np.uint32))
        r = self._write_decoder(er, _as(block_sid, np.uint64), _as(block_view, np.uint32), c, dst_cap)
        r["dstreams"] = r["dstreams"].view(SPAN_IN_DTYPE)
        return r

    def write_decoder_dev(self, emit_result, block_sid, block_view, cancel=None, dst_cap=None):
        """qh_dec_write_decoder_batch: the same over torch tensors in HBM (an
        ``emit_fields_dev`` result; block_sid int64, block_view int32, cancel
        = (int64, int32) tensors).  -> dict of tensors (dstreams as bytes).
        One host wait, for the total."""
        assert self.codec is not None
        return self._write_decoder(emit_result, block_sid, block_view, cancel, dst_cap)

    # -- blocked sections (max_blocked given): qh_dec_blocked_* / qh_qpack_dec_blocked_*

    def _blocked(self):
        if self.max_blocked is None:
            raise ValueError("the set was made without max_blocked")
        return self._be

    def _push_blocked(self, src, blocks, block_sid, block_view, emit_result, caps):
        be = self._blocked()
        ptr = be.ptr
        nblocks = be.size(block_sid)
        verdict = be.zeros(max(nblocks, 1), np.int32)

        def attempt():
            nr, nb = ctypes.c_uint64(self.nblks), ctypes.c_uint64(self.npend)
            rcap, bcap = (be.size(self.blks) // 32, be.size(self.pend)) if caps is None else caps
            rv = be.call(self._lib, "dec_blocked_push", ptr(src), ptr(blocks), ptr(block_sid),
                         ptr(block_view), ptr(emit_result["status"]), ptr(emit_result["ricnt"]),
                         nblocks, self.ntables, ptr(self.bq), ptr(self.blks), ctypes.byref(nr), rcap,
                         ptr(self.pend), ctypes.byref(nb), bcap, ptr(verdict))
            return rv, (int(nr.value), int(nb.value))

        def enlarge(needs):
            self._grow("blks", self.nblks * 32, needs[0] * 32, 4096)
            self._grow("pend", self.npend, needs[1], 4096)
        rv, (nr, nb) = be.retry("dec_blocked_push", attempt, enlarge, caps is not None)
        if rv == 0:
            self.nblks, self.npend = nr, nb
        return {"rv": rv, "verdict": verdict[:nblocks], "nblks": nr, "npend": nb}

    def push_blocked(self, src, blocks, block_sid, block_view, emit_result, caps=None):
        """After ``emit_fields`` (host form, qh_qpack_dec_blocked_push): queues
        the blocks whose status is EMIT_BLOCKED.  Every array is indexed by
        position in the emit call's sel: blocks SPAN_IN_DTYPE spans of src,
        block_sid uint64, block_view uint32 (a table's blocks consecutive),
        emit_result the emit call's dict (status, ricnt).  -> dict: verdict
        (int32: EMIT_BLOCKED queued, -101 the stream is queued already, -401
        too many blocked streams, else the block's status), rv, nblks, npend.
        The logs grow as needed; caps = (records, bytes) fixes the
        capacities instead and hands the call's return value back in rv."""
        assert self.codec is None
        er = {"status": _as(emit_result["status"], np.int32), "ricnt": _as(emit_result["ricnt"], np.uint64)}
        return self._push_blocked(_u8(src), _as(blocks, SPAN_IN_DTYPE), _as(block_sid, np.uint64),
                                  _as(block_view, np.uint32), er, caps)

    def push_blocked_dev(self, src, blocks, block_sid, block_view, emit_result, caps=None):
        """qh_dec_blocked_push_batch: the same over torch tensors in HBM (src
        uint8, blocks int64 [n, 2], block_sid int64, block_view int32, an
        ``emit_fields_dev`` result).  One host wait, for the totals."""
        assert self.codec is not None
        return self._push_blocked(src, blocks, block_sid, block_view, emit_result, caps)

    _RELEASED = (("blocks", 16), ("sid", 8), ("view", 4), ("ricnt", 8))  # (bytes per record)

    def _release_blocked(self, tsel, rel_cap, dtypes):
        """-> the result dict: blocks, sid, view, ricnt and start viewed in
        `dtypes`, the whole byte arrays kept as <name>_raw."""
        be = self._blocked()
        ptr = be.ptr
        nsel = self.ntables if tsel is None else be.size(tsel)
        fixed = rel_cap is not None
        cap = rel_cap if fixed else getattr(self, "_rel_cap", 64)
        start = be.zeros((nsel + 1) * 4)
        o = {}

        def attempt():
            # (tests: sentinel records behind a fixed capacity)
            o.update({k: be.room(cap, 4 if fixed else 0, w) for k, w in self._RELEASED})
            need = ctypes.c_uint64(0)
            rv = be.call(self._lib, "dec_blocked_release", be.list_ptr(tsel), nsel, self.ntables,
                         ptr(self.views), ptr(self.bq), ptr(self.blks), self.nblks, ptr(o["blocks"]),
                         ptr(o["sid"]), ptr(o["view"]), ptr(o["ricnt"]), ptr(start),
                         ctypes.byref(need), cap)
            return rv, int(need.value)

        def enlarge(need):
            nonlocal cap
            cap = self._rel_cap = cap_for(need, cap)
        rv, need = be.retry("dec_blocked_release", attempt, enlarge, fixed)
        n = need if rv == 0 else 0
        for (k, w), d in zip(self._RELEASED, dtypes):
            o[k + "_raw"] = o[k]
            o[k] = o[k][:n * w].view(d)
        o.update({"rv": rv, "start": start.view(dtypes[-1]), "nreleased": need, "cap": cap})
        return o

    def release_blocked(self, tsel=None, rel_cap=None):
        """After ``read_encoder`` (host form, qh_qpack_dec_blocked_release): the
        queued sections of the listed tables (uint32, each at most once; None:
        all) whose Required Insert Count the table now holds are removed.  ->
        dict: nreleased, blocks (SPAN_IN_DTYPE spans of ``pend``), sid
        (uint64), view (uint32), ricnt (uint64), the released sections of
        listed table i at [start[i], start[i + 1]) in (ricnt, arrival) order;
        rv.  blocks / view go into decode_blocks and emit_fields with src =
        ``pend``, sid / view into write_decoder.  rel_cap: a fixed capacity
        instead of growing."""
        assert self.codec is None
        return self._release_blocked(_as(tsel, np.uint32), rel_cap,
                                     (SPAN_IN_DTYPE, np.uint64, np.uint32, np.uint64, np.uint32))

    def release_blocked_dev(self, tsel=None, rel_cap=None):
        """qh_dec_blocked_release_batch: the same on the device (tsel int32 or
        None).  -> dict of tensors: blocks int64 [n, 2], sid int64, view int32,
        ricnt int64, start int32 [nsel + 1]; nreleased, rv.  One host wait."""
        import torch
        assert self.codec is not None
        o = self._release_blocked(tsel, rel_cap,
                                  (torch.int64, torch.int64, torch.int32, torch.int64, torch.int32))
        o["blocks"] = o["blocks"].reshape(-1, 2)
        return o

    @staticmethod
    def released_status(emit_result, rel):
        """The status of released blocks after their emit: -401 where a block
        came out blocked again or with another Required Insert Count than the
        one it was queued with (the reference keeps the first value; emit
        reconstructs it again).  numpy arrays or torch tensors."""
        st, ri, want = emit_result["status"], emit_result["ricnt"], rel["ricnt"]
        n = want.shape[0]
        st, ri = st[:n], ri[:n]
        if isinstance(st, np.ndarray):
            bad = (st == EMIT_BLOCKED) | ((st == 0) & (ri.view(np.uint64) != want.view(np.uint64)))
            return np.where(bad, np.int32(QH_ERR_QPACK_DECOMPRESSION_FAILED), st).astype(np.int32)
        import torch
        bad = (st == EMIT_BLOCKED) | ((st == 0) & (ri != want))
        return torch.where(bad, torch.full_like(st, QH_ERR_QPACK_DECOMPRESSION_FAILED), st)

    def _cancel_blocked(self, sid, view):
        be = self._blocked()
        ptr = be.ptr
        n = be.size(sid)
        removed = be.zeros(max(n, 1))
        rv = be.call(self._lib, "dec_blocked_cancel", ptr(sid), ptr(view), n, self.ntables, ptr(self.bq),
                     ptr(self.blks), self.nblks, ptr(removed))
        return rv, removed[:n]

    def cancel_blocked(self, cancel_sid, cancel_view, check=True):
        """Host form (qh_qpack_dec_blocked_cancel): the queued sections of the
        cancelled streams (uint64 ids, uint32 tables; a table's consecutive)
        leave the queue.  -> removed (uint8: 1 where one was queued)."""
        assert self.codec is None
        rv, removed = self._cancel_blocked(np.ascontiguousarray(cancel_sid, dtype=np.uint64),
                                           np.ascontiguousarray(cancel_view, dtype=np.uint32))
        if check:
            self._be.check(rv, "dec_blocked_cancel")
            return removed
        return rv, removed

    def cancel_blocked_dev(self, cancel_sid, cancel_view):
        """qh_dec_blocked_cancel_batch (int64 ids, int32 tables): no host wait;
        removed is 0xFF for the items of a table's second run or of a table
        out of range, which remove nothing."""
        assert self.codec is not None
        rv, removed = self._cancel_blocked(cancel_sid, cancel_view)
        self._be.check(rv, "dec_blocked_cancel")
        return removed

    _LOG_ROOMS = ((32, 128), (1, 4096))  # (records of 32 bytes, bytes: 4096 bytes at the least)

    def compact_blocked(self):
        """Replaces ``blks`` and ``pend`` by logs that hold the queued records
        of every table alone, back to back in table order, ``bq`` rebased.
        When to call is the caller's decision: compare ``nblks`` and ``npend``
        with what is queued.  A failed call leaves the object as it was."""
        be = self._blocked()
        ptr = be.ptr
        bq = be.own(self.bq)

        def call(outs):
            recs, byts = outs
            nr, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rv = be.call(self._lib, "dec_blocked_compact", None, self.ntables, self.ntables, ptr(bq),
                         ptr(self.blks), self.nblks, ptr(self.pend), self.npend, ptr(recs),
                         ctypes.byref(nr), be.size(recs) // 32, ptr(byts), ctypes.byref(nb),
                         be.size(byts))
            return rv, (int(nr.value), int(nb.value))
        (recs, byts), (nr, nb) = be.sized("dec_blocked_compact", call, self._LOG_ROOMS, be.zeros)
        self.bq, self.blks, self.pend, self.nblks, self.npend = bq, recs, byts, nr, nb

    def blocked_records(self):
        """-> (bq DEC_BLKS_DTYPE [ntables], blks DEC_BLK_DTYPE [nblks], pend
        uint8 [npend]): host copies of the queue state."""
        h = self._blocked().host
        return (h(self.bq).view(DEC_BLKS_DTYPE), h(self.blks[:self.nblks * 32]).view(DEC_BLK_DTYPE),
                h(self.pend[:self.npend]))

    # -- sections in pieces (max_section_bytes given): qh_dec_partial_* / qh_qpack_dec_partial_*

    def _partial(self):
        if self.max_section_bytes is None:
            raise ValueError("the set was made without max_section_bytes")
        return self._be

    _DONE = (("done_blocks", 16), ("done_sid", 8), ("done_view", 4))  # (bytes per section)

    def _push_pieces(self, src, pieces, piece_sid, piece_view, fin, caps, dtypes):
        be = self._partial()
        ptr = be.ptr
        n = be.size(piece_sid)
        fixed = caps is not None
        verdict = be.zeros(max(n, 1), np.int32)
        o = {k: be.zeros(max(n, 1) * w) for k, w in self._DONE}
        dcap = caps[2] if fixed else getattr(self, "_done_cap", 4096)

        def attempt():
            # (tests: sentinel bytes behind a fixed capacity)
            o["done"] = be.room(dcap, 64) if fixed else be.empty(dcap)
            nr, nb = ctypes.c_uint64(self.nparts), ctypes.c_uint64(self.nheld)
            dn, nd = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rcap, bcap = caps[:2] if fixed else (be.size(self.parts) // 32, be.size(self.held))
            rv = be.call(self._lib, "dec_partial_push", ptr(src), ptr(pieces), ptr(piece_sid),
                         ptr(piece_view), ptr(fin), n, self.ntables, ptr(self.pq), ptr(self.parts),
                         ctypes.byref(nr), rcap, ptr(self.held), ctypes.byref(nb), bcap, ptr(verdict),
                         ptr(o["done"]), dcap, ctypes.byref(dn), ptr(o["done_blocks"]),
                         ptr(o["done_sid"]), ptr(o["done_view"]), ctypes.byref(nd))
            return rv, (int(nr.value), int(nb.value), int(dn.value), int(nd.value))

        def enlarge(needs):
            nonlocal dcap
            self._grow("parts", self.nparts * 32, needs[0] * 32, 4096)
            self._grow("held", self.nheld, needs[1], 4096)
            dcap = self._done_cap = cap_for(needs[2], dcap)
        rv, (nr, nb, dn, nd) = be.retry("dec_partial_push", attempt, enlarge, fixed)
        if rv == 0:
            self.nparts, self.nheld = nr, nb
        k = nd if rv == 0 else 0
        for (name, w), d in zip(self._DONE, dtypes):
            o[name + "_raw"] = o[name]
            o[name] = o[name][:k * w].view(d)
        o.update({"rv": rv, "verdict": verdict[:n], "nparts": nr, "nheld": nb, "done_need": dn, "ndone": nd})
        return o

    def push_pieces(self, src, pieces, piece_sid, piece_view, fin, caps=None):
        """Pieces of field sections as they arrive (host form,
        qh_qpack_dec_partial_push): pieces SPAN_IN_DTYPE spans of src,
        piece_sid uint64, piece_view uint32 (a table's pieces consecutive, a
        stream at most once per call), fin uint8 (the section ends with the
        piece).  -> dict: verdict (int32: PART_DONE the section is complete,
        PART_KEPT held, -101 the stream came earlier in the call, -109 longer
        than max_section_bytes: dropped), and the finished sections done
        (uint8), done_blocks (SPAN_IN_DTYPE spans of done), done_sid
        (uint64), done_view (uint32), ndone, done_need; rv, nparts, nheld.
        done / done_blocks / done_view go into decode_blocks and emit_fields,
        done_sid / done_view into push_blocked and write_decoder.  The logs
        grow as needed; caps = (records, held bytes, done bytes) fixes the
        capacities instead and hands the call's return value back in rv."""
        assert self.codec is None
        return self._push_pieces(_u8(src), _as(pieces, SPAN_IN_DTYPE), _as(piece_sid, np.uint64),
                                 _as(piece_view, np.uint32), _as(fin, np.uint8), caps,
                                 (SPAN_IN_DTYPE, np.uint64, np.uint32))

    def push_pieces_dev(self, src, pieces, piece_sid, piece_view, fin, caps=None):
        """qh_dec_partial_push_batch: the same over torch tensors in HBM (src
        uint8, pieces int64 [n, 2], piece_sid int64, piece_view int32, fin
        uint8).  -> dict of tensors (done_blocks int64 [ndone, 2], done_sid
        int64, done_view int32).  One host wait, for the totals."""
        import torch
        assert self.codec is not None
        o = self._push_pieces(src, pieces, piece_sid, piece_view, fin, caps,
                              (torch.int64, torch.int64, torch.int32))
        o["done_blocks"] = o["done_blocks"].reshape(-1, 2)
        return o

    def _cancel_pieces(self, sid, view):
        be = self._partial()
        ptr = be.ptr
        n = be.size(sid)
        removed = be.zeros(max(n, 1))
        rv = be.call(self._lib, "dec_partial_cancel", ptr(sid), ptr(view), n, self.ntables, ptr(self.pq),
                     ptr(self.parts), self.nparts, ptr(removed))
        return rv, removed[:n]

    def cancel_pieces(self, cancel_sid, cancel_view, check=True):
        """Host form (qh_qpack_dec_partial_cancel), on a stream reset: the held
        bytes of the cancelled streams (uint64 ids, uint32 tables; a table's
        consecutive) are dropped.  -> removed (uint8: 1 where some were held)."""
        assert self.codec is None
        rv, removed = self._cancel_pieces(np.ascontiguousarray(cancel_sid, dtype=np.uint64),
                                          np.ascontiguousarray(cancel_view, dtype=np.uint32))
        if check:
            self._be.check(rv, "dec_partial_cancel")
            return removed
        return rv, removed

    def cancel_pieces_dev(self, cancel_sid, cancel_view):
        """qh_dec_partial_cancel_batch (int64 ids, int32 tables): no host wait;
        removed is 0xFF for the items of a table's second run or of a table
        out of range, which remove nothing."""
        assert self.codec is not None
        rv, removed = self._cancel_pieces(cancel_sid, cancel_view)
        self._be.check(rv, "dec_partial_cancel")
        return removed

    def compact_pieces(self):
        """Replaces ``parts`` and ``held`` by logs that hold the unfinished
        sections of every table alone, back to back in table order, ``pq``
        rebased.  When to call is the caller's decision: compare ``nheld``
        with what is held; every continued section leaves its previous copy
        dead, so this log fills faster than the blocked one.  A failed call
        leaves the object as it was."""
        be = self._partial()
        ptr = be.ptr
        pq = be.own(self.pq)

        def call(outs):
            recs, byts = outs
            nr, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rv = be.call(self._lib, "dec_partial_compact", None, self.ntables, self.ntables, ptr(pq),
                         ptr(self.parts), self.nparts, ptr(self.held), self.nheld, ptr(recs),
                         ctypes.byref(nr), be.size(recs) // 32, ptr(byts), ctypes.byref(nb),
                         be.size(byts))
            return rv, (int(nr.value), int(nb.value))
        (recs, byts), (nr, nb) = be.sized("dec_partial_compact", call, self._LOG_ROOMS, be.zeros)
        self.pq, self.parts, self.held, self.nparts, self.nheld = pq, recs, byts, nr, nb

    def piece_records(self):
        """-> (pq DEC_PARTS_DTYPE [ntables], parts DEC_PART_DTYPE [nparts],
        held uint8 [nheld]): host copies of the unfinished sections' state."""
        h = self._partial().host
        return (h(self.pq).view(DEC_PARTS_DTYPE), h(self.parts[:self.nparts * 32]).view(DEC_PART_DTYPE),
                h(self.held[:self.nheld]))

    def compact(self, extra_views=None):
        """Compacts the log (qh_dtables_compact_batch on the device form,
        qh_qpack_dtables_compact on the numpy form): the live records of
        every table copied to fresh ``entries`` / ``dyn_bytes`` arrays, bytes
        unshared, ``views`` rewritten, ``nentries`` / ``nbytes`` the compacted
        lengths; ``keys()`` recomputes over the new log.  `extra_views`
        (VIEW_DTYPE records or their bytes; a uint8 tensor on the device
        form): older snapshots of tables the caller still needs, each given a
        region of its own after the set's views; -> their rewritten copies
        (None without extra_views).  Copies of ``views`` and of the old
        arrays taken before the call stay valid together.  When to call is the
        caller's decision: compare ``nentries`` and ``nbytes`` with what the
        tables can hold.  A failed call leaves the object as it was."""
        be = self._be
        ptr = be.ptr
        if extra_views is None:
            views = be.own(self.views)
        elif be.dev:
            views = be.torch.cat([self.views, extra_views.reshape(-1).view(be.torch.uint8)])
        else:
            views = np.concatenate([self.views,
                                    np.ascontiguousarray(extra_views).view(np.uint8).reshape(-1)])
        nv = be.size(views) // VIEW_DTYPE.itemsize
        status = be.empty(max(nv, 1), np.int32)

        def call(outs):
            ents, byts = outs
            ne, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            rv = be.call(self._lib, "dtables_compact", nv, ptr(views), ptr(self.entries), self.nentries,
                         ptr(self.dyn_bytes), self.nbytes, ptr(ents), ctypes.byref(ne),
                         be.size(ents) // 32, ptr(byts), ctypes.byref(nb), be.size(byts), ptr(status))
            return rv, (int(ne.value), int(nb.value))
        (ents, byts), (ne, nb) = be.sized("dtables_compact", call, self._LOG_ROOMS, be.empty)
        own = self.ntables * VIEW_DTYPE.itemsize
        self.views = views if extra_views is None else be.own(views[:own])
        self.entries, self.dyn_bytes, self.nentries, self.nbytes = ents, byts, ne, nb
        self._nkeys = 0  # (keys depend on content alone: keys() computes them over the new log)
        self._index_recs = None  # (an index names records by position: index() builds it again)
        if not be.dev:
            self._keys = be.empty(0)  # (an array handed out by keys() before stays as it was)
        return None if extra_views is None else be.own(views[own:])

    def keys(self):
        """The log's keys (DYN_KEY_DTYPE records; a uint8 tensor of nentries *
        16 bytes on the device), extended over the tail appended since the
        last call (qh_dyn_keys_batch / qh_qpack_dyn_keys)."""
        n, be = self.nentries, self._be
        ptr = be.ptr
        self._grow("_keys", self._nkeys * 16, n * 16, 4096)
        if n > self._nkeys:
            be.check(be.call(self._lib, "dyn_keys", ptr(self.entries), n, ptr(self.dyn_bytes),
                             self.nbytes, self._nkeys, n - self._nkeys, ptr(self._keys)), "dyn_keys")
            self._nkeys = n
        keys = self._keys[:n * 16]
        return keys if be.dev else keys.view(DYN_KEY_DTYPE)

    def index(self, tsel=None, max_buckets=0):
        """The hashed index over the tables' keys (qh_dyn_index_batch /
        qh_qpack_dyn_index): built for the tables `tsel` (uint32 indices;
        None: every table, from an empty slots array), the other tables'
        records and regions kept.  -> {"recs", "slots", "nslots"} for the
        planners' ``index=`` (uint8 tensors on the device form;
        DYN_INDEX_REC_DTYPE records and uint32 slots on the host).  A table's
        index is built only here: after ``compact()`` every index has to be
        built again (the set drops what it kept), and after more inserts an
        older one stays usable until the caller asks for a new one."""
        be = self._be
        ptr = be.ptr
        keys = self.keys()
        if not be.dev:
            tsel = _as(tsel, np.uint32)
        if getattr(self, "_index_recs", None) is None or tsel is None:
            self._index_recs, self._index_slots, self._nslots = be.zeros(max(self.ntables, 1) * 48), None, 0
        keep, old, recs = self._nslots, self._index_slots, self._index_recs
        nsel = 0 if tsel is None else be.size(tsel)

        def call(outs):
            (slots,) = outs
            if slots is not None and keep:
                slots[:keep * 4] = old[:keep * 4]
            ns = ctypes.c_uint64(keep)
            rv = be.call(self._lib, "dyn_index", ptr(self.views), self.ntables, be.list_ptr(tsel), nsel,
                         ptr(keys), self.nentries, max_buckets, ptr(recs), ptr(slots), ctypes.byref(ns),
                         be.size(slots) // 4)
            return rv, (int(ns.value),)
        (self._index_slots,), (self._nslots,) = be.sized("dyn_index", call, ((4, 1024),), be.empty)
        if be.dev:
            return {"recs": recs, "slots": self._index_slots, "nslots": self._nslots}
        return {"recs": recs.view(DYN_INDEX_REC_DTYPE)[:self.ntables],
                "slots": self._index_slots.view(np.uint32), "nslots": self._nslots}


class EncoderSet:
    """The QPACK encoders of `n` connections with dynamic-table inserts over
    one log (qh_qpack_encode_conns / qh_encode_conns_batch): `n` fresh
    encoders of hard maximum capacity `hard_max` (a scalar, or one value per
    connection) at capacity 0, as nghttp3_qpack_encoder_new leaves them.

    The object owns the views, acct and enc records, the log and its keys,
    grows them on QH_ERR_NOMEM and calls again, as DynamicTableSet does.
    With ``device=None`` they are numpy arrays and ``encode`` is the host
    twin; with a device index they are torch tensors there and
    ``encode_dev(codec, ...)`` runs the walk on the GPU.

    With ``refs=True`` the object also owns the acknowledgement state (``rv``,
    one ENC_REFS_DTYPE record per connection, and the reference log
    ``refs``): ``encode`` / ``encode_dev`` take ``stream_ids=`` and run
    sec-flags -> encode -> record, ``read_decoder`` / ``read_decoder_dev``
    apply the peer's decoder streams, ``refs_records()`` reads the state back
    and ``compact_refs()`` gives the log's abandoned regions back.  Without
    it acknowledgements are the caller's: between calls it edits
    ``enc_records()`` (krcnt, pin_min, nblocked, nstreams) and stores them
    back with ``set_enc_records``.

    With ``streams=True`` (and ``refs=True``) the object also keeps each
    connection's decoder stream as it arrives (``ustreams``, a HeldStreams):
    ``feed_decoder`` / ``feed_decoder_dev`` take whatever bytes have come and
    hold a cut instruction until the rest follows.

    With ``index=True`` the object also owns a hashed index per connection
    (``recs``, one ENC_INDEX_REC_DTYPE record each, and ``slots``):
    ``encode`` / ``encode_dev`` then make the indexed calls
    (qh_qpack_encode_conns_indexed / qh_encode_conns_indexed_batch), whose
    outputs are the un-indexed ones byte for byte while a lookup walks a hash
    chain instead of every live key.  The regions are made by the first call
    (``init_index``); a connection with fewer than `index_min_entries`
    possible entries (hard_max / 32) is scanned as before, and
    `index_max_buckets` (0: no limit) cuts the bucket counts.
    ``index_records()`` and ``index_slots()`` read the index back."""

    def __init__(self, hard_max, n: int, max_blocked=0, immediate_ack: bool = False, device=None,
                 strat_none: bool = False, refs: bool = False, streams: bool = False,
                 index: bool = False, index_min_entries: int = 0, index_max_buckets: int = 0):
        if streams and not refs:
            raise ValueError("streams=True needs refs=True: the decoder stream is read into the reference log")
        self._lib = _load()
        self.n = int(n)
        self.has_refs = bool(refs)
        self.nrefs = 0
        hm = np.broadcast_to(np.asarray(hard_max, dtype=np.uint64), (self.n,))
        mb = np.broadcast_to(np.asarray(max_blocked, dtype=np.uint64), (self.n,))
        flags = (ENC_IMMEDIATE_ACK if immediate_ack else 0) | (ENC_STRAT_NONE if strat_none else 0)
        views = np.zeros(max(self.n, 1), dtype=VIEW_DTYPE)[:self.n]
        acct = np.zeros(max(self.n, 1), dtype=ACCT_DTYPE)[:self.n]
        enc = np.zeros(max(self.n, 1), dtype=ENC_STATE_DTYPE)[:self.n]
        v1, a1, e1 = (np.zeros(1, dtype=d) for d in (VIEW_DTYPE, ACCT_DTYPE, ENC_STATE_DTYPE))
        for t in range(self.n):
            self._lib.qh_enc_state_init(int(hm[t]), int(mb[t]), flags, _vp(v1), _vp(a1), _vp(e1))
            views[t], acct[t], enc[t] = v1[0], a1[0], e1[0]
        self.nentries = 0
        self.nbytes = 0
        self.device = device
        be = self._be = Backend(None if device is None else "cuda:%d" % int(device))
        arrays = {"views": views, "acct": acct, "enc": enc}
        if refs:  # (a fresh connection's record is all zeros: qh_enc_refs_init)
            arrays["rv"] = np.zeros(max(self.n, 1), dtype=ENC_REFS_DTYPE)[:self.n]
            arrays["refs"] = np.zeros(0, dtype=ENC_REF_DTYPE)
        for k, a in arrays.items():
            setattr(self, k, be.put(a.view(np.uint8).copy()))
        for k in ("entries", "dyn_bytes", "keys"):
            setattr(self, k, be.empty(0))
        self.ustreams = HeldStreams(self._lib, be, self.n) if streams else None
        # the index: its regions are made by the first call, which has the device form's codec
        self.has_index, self._index_ready = bool(index), False
        self._index_opts = (int(index_min_entries), int(index_max_buckets))
        self.nslots = 0
        self.recs, self.slots = be.zeros(max(self.n, 1) * ENC_INDEX_REC_DTYPE.itemsize), be.empty(0)

    # -- the index (index=True): qh_qpack_enc_index_init / qh_enc_index_init_batch

    def init_index(self, codec: HuffmanBatchCodec | None = None, tsel=None, slots_cap=None):
        """Sizes and allocates the index regions of connections `tsel` (uint32
        / int32 indices; None: all) behind the slots in use, and links the
        entries live now: a set made without ``index=True`` adopts an index
        this way mid-life.  ``encode`` / ``encode_dev`` call it once by
        themselves.  slots grows on QH_ERR_NOMEM (slots_cap: a fixed capacity
        instead, for tests; the call is then made once).  -> (the call's
        return value, the slots in use or needed)."""
        be = self._be
        ptr = be.ptr
        nsel = 0 if tsel is None else be.size(tsel)
        self.has_index = self._index_ready = True

        def attempt():
            ns = ctypes.c_uint64(self.nslots)
            cap = be.size(self.slots) // 4 if slots_cap is None else slots_cap
            rv = be.call(self._lib, "enc_index_init", ptr(self.views), ptr(self.acct), self.n,
                         be.list_ptr(tsel), nsel, ptr(self.keys), self.nentries, self._index_opts[0],
                         self._index_opts[1], ptr(self.recs), ptr(self.slots), ctypes.byref(ns), cap,
                         codec=codec)
            return rv, int(ns.value)
        rv, ns = be.retry("enc_index_init", attempt,
                          lambda need: self._grow("slots", self.nslots * 4, need * 4, 4096),
                          slots_cap is not None)
        if rv == 0:
            self.nslots = ns
        return rv, ns

    def index_records(self):
        """-> ENC_INDEX_REC_DTYPE [n], a numpy copy."""
        return self._host("recs", np.uint8)[:self.n * ENC_INDEX_REC_DTYPE.itemsize].view(ENC_INDEX_REC_DTYPE)

    def index_slots(self):
        """-> uint32 [nslots], a numpy copy of the slots in use."""
        return self._host("slots", np.uint8)[:self.nslots * 4].view(np.uint32)

    # -- state access (numpy copies; the device form copies through the host)

    def _host(self, name, dtype):
        return self._be.host(getattr(self, name)).view(dtype)

    def _store(self, name, recs):
        setattr(self, name, self._be.put(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()))

    def view_records(self):
        return self._host("views", VIEW_DTYPE)

    def acct_records(self):
        return self._host("acct", ACCT_DTYPE)

    def enc_records(self):
        return self._host("enc", ENC_STATE_DTYPE)

    def set_enc_records(self, recs):
        self._store("enc", np.ascontiguousarray(recs, dtype=ENC_STATE_DTYPE))

    def log(self):
        """-> (entries DYN_ENTRY_DTYPE, bytes uint8, keys DYN_KEY_DTYPE), numpy copies."""
        return (self._host("entries", np.uint8)[:self.nentries * 32].view(DYN_ENTRY_DTYPE),
                self._host("dyn_bytes", np.uint8)[:self.nbytes],
                self._host("keys", np.uint8)[:self.nentries * 16].view(DYN_KEY_DTYPE))

    def set_capacity(self, caps):
        """nghttp3_qpack_encoder_set_max_dtable_capacity per connection (a
        scalar or one value each); the instruction is written by the next
        call that encodes a section of the connection."""
        caps = np.broadcast_to(np.asarray(caps, dtype=np.uint64), (self.n,))
        acct, enc = self.acct_records(), self.enc_records()
        a1, e1 = np.zeros(1, dtype=ACCT_DTYPE), np.zeros(1, dtype=ENC_STATE_DTYPE)
        for t in range(self.n):
            a1[0], e1[0] = acct[t], enc[t]
            self._lib.qh_enc_state_set_capacity(_vp(e1), _vp(a1), int(caps[t]))
            acct[t], enc[t] = a1[0], e1[0]
        self._store("acct", acct)
        self._store("enc", enc)

    _grow = grow

    def _call(self, codec, plain, strs, nfields, nvflags, field_start, nsections, sec_flags,
              conn_start, nconns, tsel, caps=None):
        """One call, grown and repeated on QH_ERR_NOMEM (`caps`: fixed
        (entries, bytes, dst, edst) capacities instead, for tests; the call is
        then made once and its return value and needs handed back)."""
        be = self._be
        ptr, new = be.ptr, be.zeros
        if self.has_index and not self._index_ready:
            self.init_index(codec)
        # (the indexed stem's three arguments more; the regions never move, so they are fixed here)
        index = (ptr(self.recs), ptr(self.slots), self.nslots) if self.has_index else ()
        lines = new(max(nfields, 1) * 24)
        prefixes = new(max(nsections, 1) * 24)
        mx, mn = new(max(nsections, 1) * 8), new(max(nsections, 1) * 8)
        sections = new(max(nsections, 1) * 16)
        estreams = new(max(nconns, 1) * 16)
        status = new(max(nconns, 1) * 4)
        # (the output buffers start at the sizes the last call needed)
        dst_cap, edst_cap = getattr(self, "_out_caps", (4096, 4096))
        fixed = caps is not None
        pad = 64 if fixed else 0
        if fixed:
            # exactly the given room, with 64 sentinel bytes (0xA5) behind it
            for name, have, cap in (("entries", self.nentries * 32, caps[0] * 32),
                                    ("keys", self.nentries * 16, caps[0] * 16),
                                    ("dyn_bytes", self.nbytes, caps[1])):
                a = new(cap + pad)
                a[:] = 0xA5
                a[:have] = getattr(self, name)[:have]
                setattr(self, name, a)
            dst_cap, edst_cap = caps[2], caps[3]
        dst = edst = None

        def attempt():
            nonlocal dst, edst
            dst, edst = be.room(dst_cap, pad), be.room(edst_cap, pad)
            ne, nb = ctypes.c_uint64(self.nentries), ctypes.c_uint64(self.nbytes)
            dn, en = ctypes.c_uint64(0), ctypes.c_uint64(0)
            ecap = caps[0] if fixed else min(be.size(self.entries) // 32, be.size(self.keys) // 16)
            bcap = caps[1] if fixed else be.size(self.dyn_bytes)
            rv = be.call(self._lib, "encode_conns" + ("_indexed" if index else ""), ptr(plain), ptr(strs),
                         nfields, ptr(nvflags),
                         ptr(field_start), nsections, ptr(sec_flags), ptr(conn_start), nconns,
                         be.list_ptr(tsel), self.n, ptr(self.views), ptr(self.acct), ptr(self.enc),
                         ptr(self.entries), ctypes.byref(ne), ecap, ptr(self.dyn_bytes),
                         ctypes.byref(nb), bcap, ptr(self.keys), ptr(lines), ptr(prefixes), ptr(mx),
                         ptr(mn), ptr(dst), dst_cap, ptr(sections), ctypes.byref(dn), ptr(edst),
                         edst_cap, ptr(estreams), ctypes.byref(en), ptr(status), *index, codec=codec)
            return rv, (int(ne.value), int(nb.value), int(dn.value), int(en.value))

        def enlarge(needs):
            nonlocal dst_cap, edst_cap
            self._grow("entries", self.nentries * 32, needs[0] * 32, 4096)
            self._grow("keys", self.nentries * 16, needs[0] * 16, 2048)
            self._grow("dyn_bytes", self.nbytes, needs[1], 4096)
            dst_cap, edst_cap = cap_for(needs[2], dst_cap), cap_for(needs[3], edst_cap)
            self._out_caps = (dst_cap, edst_cap)
        rv, needs = be.retry("encode_conns", attempt, enlarge, fixed, tries=3)
        if rv == 0:
            self.nentries, self.nbytes = needs[0], needs[1]
        return {"rv": rv, "needs": needs, "lines": lines, "prefixes": prefixes, "max_cnt": mx,
                "min_cnt": mn, "dst": dst, "sections": sections, "edst": edst, "estreams": estreams,
                "status": status, "nfields": nfields, "nsections": nsections, "nconns": nconns}

    # -- acknowledgements (refs=True): the calls of csrc/qh_ack.c / qh_ack.inc

    def _sec_flags(self, codec, sids, conn_start, nsections, nconns, tsel):
        """qh_qpack_enc_sec_flags / qh_enc_sec_flags_batch -> (sec_flags uint8,
        status int32 as bytes), arrays of the object's kind."""
        be = self._be
        ptr = be.ptr
        flags, status = be.zeros(max(nsections, 1)), be.zeros(max(nconns, 1) * 4)
        rv = be.call(self._lib, "enc_sec_flags", ptr(sids), nsections, ptr(conn_start), nconns,
                     be.list_ptr(tsel), self.n, ptr(self.enc), ptr(self.rv), ptr(self.refs),
                     self.nrefs, ptr(flags), ptr(status), codec=codec)
        be.check(rv, "enc_sec_flags")
        return flags[:nsections], status

    def _record(self, codec, sids, conn_start, nsections, nconns, tsel, r, refs_cap=None):
        """qh_qpack_enc_refs_record / qh_enc_refs_record_batch after an encode
        call with result r; the log grows on QH_ERR_NOMEM (refs_cap: a fixed
        capacity instead, for tests).  -> (the call's return value, nrefs)."""
        be = self._be
        ptr = be.ptr

        def attempt():
            nr = ctypes.c_uint64(self.nrefs)
            cap = be.size(self.refs) // 32 if refs_cap is None else refs_cap
            rv = be.call(self._lib, "enc_refs_record", ptr(sids), nsections, ptr(conn_start), nconns,
                         be.list_ptr(tsel), self.n, ptr(r["max_cnt"]), ptr(r["min_cnt"]),
                         ptr(r["status"]), ptr(self.enc), ptr(self.rv), ptr(self.refs),
                         ctypes.byref(nr), cap, codec=codec)
            return rv, int(nr.value)
        rv, nr = be.retry("enc_refs_record", attempt,
                          lambda need: self._grow("refs", self.nrefs * 32, need * 32, 4096),
                          refs_cap is not None)
        if rv == 0:
            self.nrefs = nr
        return rv, nr

    def _read_decoder(self, codec, src, streams, tsel):
        assert self.has_refs
        be = self._be
        ptr = be.ptr
        nsel = self.n if tsel is None else be.size(tsel)
        status = be.empty(max(nsel, 1), np.int32)
        consumed = be.empty(max(nsel, 1), np.int32)
        rv = be.call(self._lib, "enc_read_decoder", ptr(src), ptr(streams), be.list_ptr(tsel), nsel,
                     self.n, ptr(self.views), ptr(self.enc), ptr(self.rv), ptr(self.refs), self.nrefs,
                     ptr(status), ptr(consumed), codec=codec)
        be.check(rv, "enc_read_decoder")
        return status[:nsel], consumed[:nsel]

    def read_decoder(self, src, streams, tsel=None):
        """Decoder-stream bytes applied on the host (qh_qpack_enc_read_decoder):
        stream p is src[streams[p].off, + len) (src uint8, streams
        SPAN_IN_DTYPE, tsel uint32 or None for stream p -> connection p).
        -> (status int32, consumed uint32): per stream 0 or the first failing
        instruction's error (-403; -108 once the connection is bad), and the
        bytes of complete, applied instructions."""
        status, consumed = self._read_decoder(None, _u8(src), _as(streams, SPAN_IN_DTYPE),
                                              _as(tsel, np.uint32))
        return status, consumed.view(np.uint32)

    def read_decoder_dev(self, codec: HuffmanBatchCodec, src, streams, tsel=None):
        """qh_enc_read_decoder_batch: the same over torch tensors in HBM (src
        uint8, streams int64 [nsel, 2] as SPAN_IN_DTYPE records, tsel int32).
        -> (status int32, consumed int32) tensors.  Asynchronous on the codec
        stream, no host wait."""
        return self._read_decoder(codec, src, streams, tsel)

    def _ustreams(self):
        if self.ustreams is None:
            raise ValueError("the set was made without streams=True")
        return self.ustreams

    def apply_settings(self, cs, csel=None, codec: HuffmanBatchCodec | None = None):
        """The peer's SETTINGS as ``h3_uni_read`` left them in the connection
        records `cs` (H3_CONN_DTYPE as bytes, of this set's backend) put to
        the encoders of connections `csel` (None: all): the table capacity as
        ``set_capacity`` would, max_blocked = min(100, the peer's value)
        (qh_qpack_h3_settings_apply; with the device form's codec
        qh_h3_settings_apply_batch, no host wait)."""
        be = self._be
        if isinstance(cs, np.ndarray) and cs.dtype == H3_CONN_DTYPE:
            cs = cs.view(np.uint8)
        rv = be.call(self._lib, "h3_settings_apply", be.ptr(cs), be.list_ptr(csel),
                     0 if csel is None else be.size(csel), self.n, be.ptr(self.acct), be.ptr(self.enc),
                     codec=codec)
        be.check(rv, "h3_settings_apply")

    def feed_decoder(self, src, pieces, tsel=None):
        """Decoder-stream bytes as they arrive (host form): piece p is the new
        bytes of connection tsel[p]'s stream (None: connection p), cut
        anywhere.  Runs join -> ``read_decoder`` -> keep.  -> status int32
        per piece (0, -403, -108 once the connection is bad)."""
        assert self.device is None
        return self._ustreams().feed(lambda log, joined, sel: self._read_decoder(None, log, joined, sel),
                                  _u8(src), _as(pieces, SPAN_IN_DTYPE), _as(tsel, np.uint32), 0, 0)

    def feed_decoder_dev(self, codec: HuffmanBatchCodec, src, pieces, tsel=None):
        """The same over torch tensors in HBM: qh_ustream_join_batch,
        qh_enc_read_decoder_batch, qh_ustream_keep_batch.  One host wait, for
        the join's total."""
        return self._ustreams().feed(lambda log, joined, sel: self._read_decoder(codec, log, joined, sel),
                                  src, pieces, tsel, 0, 0, codec=codec)

    def compact_streams(self, codec: HuffmanBatchCodec | None = None):
        """Replaces the decoder streams' log by one that holds the cut
        instructions alone."""
        self._ustreams().compact(codec)

    def stream_records(self):
        """-> (us USTREAM_DTYPE [n], log uint8 [nlog]), numpy copies."""
        return self._ustreams().records()

    def refs_records(self):
        """-> (rv ENC_REFS_DTYPE [n], refs ENC_REF_DTYPE [nrefs]), numpy copies:
        connection t's unacknowledged sections are refs[rv[t].base, + rv[t].n)."""
        assert self.has_refs
        return (self._host("rv", ENC_REFS_DTYPE),
                self._host("refs", np.uint8)[:self.nrefs * 32].view(ENC_REF_DTYPE))

    def compact_refs(self, codec: HuffmanBatchCodec | None = None):
        """The reference log replaced by one that holds every connection's
        references back to back, in connection order
        (qh_qpack_enc_refs_compact; with the device form's codec
        qh_enc_refs_compact_batch)."""
        assert self.has_refs
        be = self._be
        ptr = be.ptr

        def call(outs):
            nr = ctypes.c_uint64(0)
            rv = be.call(self._lib, "enc_refs_compact", None, self.n, self.n, ptr(self.rv),
                         ptr(self.refs), self.nrefs, ptr(outs[0]), ctypes.byref(nr),
                         be.size(outs[0]) // 32, codec=codec)
            return rv, (int(nr.value),)
        (self.refs,), (self.nrefs,) = be.sized("enc_refs_compact", call, ((32, 128),), be.zeros)

    def _encode(self, codec, plain, strs, field_start, conn_start, nvflags, sec_flags, tsel, caps, sids):
        """sec-flags -> encode -> record with stream ids, the encode call alone
        without; arrays of the object's kind in and out."""
        nfields, nsections = int(strs.shape[0]) // 2, int(field_start.shape[0]) - 1
        nconns = int(conn_start.shape[0]) - 1
        call = lambda flags: self._call(codec, plain, strs, nfields, nvflags, field_start, nsections,
                                        flags, conn_start, nconns, tsel, caps)
        if sids is None:
            return call(sec_flags)
        if sec_flags is not None:
            raise ValueError("pass stream_ids or sec_flags, not both")
        if not self.has_refs:
            raise ValueError("stream_ids needs an EncoderSet made with refs=True")
        flags, st = self._sec_flags(codec, sids, conn_start, nsections, nconns, tsel)
        r = call(flags)
        r["sec_flags"], r["sec_status"] = flags, st
        if r["rv"] == 0:
            self._record(codec, sids, conn_start, nsections, nconns, tsel, r)
        return r

    def encode(self, plain, strs, field_start, conn_start, nvflags=None, sec_flags=None, tsel=None,
               caps=None, stream_ids=None):
        """The host twin (qh_qpack_encode_conns) over numpy arrays: plain
        uint8, strs SPAN_IN_DTYPE (two per field), field_start / conn_start
        uint32, nvflags / sec_flags uint8 or None, tsel uint32 or None.
        -> dict of numpy arrays: lines (FIELD_LINE_DTYPE), prefixes
        (PREFIX_DTYPE), max_cnt, min_cnt (uint64), dst (uint8, the sections'
        bytes), sections (SPAN_IN_DTYPE), edst (uint8), estreams
        (SPAN_IN_DTYPE, one per listed connection), status (int32).
        stream_ids (refs=True; uint64, one per section, instead of sec_flags):
        the flags come from the reference log (qh_qpack_enc_sec_flags; the
        result gains sec_flags and sec_status) and the call's references are
        recorded after it (qh_qpack_enc_refs_record)."""
        assert self.device is None
        r = self._encode(None, _u8(plain), _as(strs, SPAN_IN_DTYPE), _as(field_start, np.uint32),
                         _as(conn_start, np.uint32), _as(nvflags, np.uint8), _as(sec_flags, np.uint8),
                         _as(tsel, np.uint32), caps, _as(stream_ids, np.uint64))
        return self._unpack(r, lambda a: a)

    def encode_dev(self, codec: HuffmanBatchCodec, plain, strs, field_start, conn_start,
                   nvflags=None, sec_flags=None, tsel=None, caps=None, stream_ids=None):
        """qh_encode_conns_batch: the same over torch tensors in HBM (plain
        uint8, strs int64 [2 nfields, 2] as SPAN_IN_DTYPE records,
        field_start / conn_start / tsel int32, nvflags / sec_flags uint8,
        stream_ids int64: qh_enc_sec_flags_batch before the call and
        qh_enc_refs_record_batch after it).
        -> the same dict, of tensors viewed as bytes (``to_host`` converts)."""
        assert self.device is not None
        return self._encode(codec, plain, strs, field_start, conn_start, nvflags, sec_flags, tsel, caps,
                            stream_ids)

    @staticmethod
    def _unpack(r, host):
        nf, ns, nc = r["nfields"], r["nsections"], r["nconns"]
        out = dict(r)
        out["lines"] = host(r["lines"])[:nf * 24].view(FIELD_LINE_DTYPE)
        out["prefixes"] = host(r["prefixes"])[:ns * 24].view(PREFIX_DTYPE)
        out["max_cnt"] = host(r["max_cnt"])[:ns * 8].view(np.uint64)
        out["min_cnt"] = host(r["min_cnt"])[:ns * 8].view(np.uint64)
        out["sections"] = host(r["sections"])[:ns * 16].view(SPAN_IN_DTYPE)
        out["estreams"] = host(r["estreams"])[:nc * 16].view(SPAN_IN_DTYPE)
        out["status"] = host(r["status"])[:nc * 4].view(np.int32)
        out["dst"], out["edst"] = host(r["dst"]), host(r["edst"])  # (needs[2], needs[3] bytes)
        if "sec_status" in r:
            out["sec_flags"] = host(r["sec_flags"])[:ns]
            out["sec_status"] = host(r["sec_status"])[:nc * 4].view(np.int32)
        return out

    @classmethod
    def to_host(cls, r):
        """An ``encode_dev`` result as ``encode`` returns it (numpy)."""
        return cls._unpack(r, lambda t: t.cpu().numpy())


def dyn_keys(entries, dyn_bytes, first: int = 0, keys=None):
    """qh_qpack_dyn_keys: the keys (DYN_KEY_DTYPE) of the log (entries
    DYN_ENTRY_DTYPE, dyn_bytes).  `keys` holds those of entries [0, first)
    already; the rest is computed and the whole array returned."""
    lib = _load()
    ents = np.ascontiguousarray(entries, dtype=DYN_ENTRY_DTYPE)
    byts = _u8(dyn_bytes)
    out = np.zeros(max(ents.size, 1), dtype=DYN_KEY_DTYPE)
    if first:
        out[:first] = np.ascontiguousarray(keys, dtype=DYN_KEY_DTYPE)[:first]
    _lib.check(lib.qh_qpack_dyn_keys(_vp(ents), ents.size, _vp(byts), byts.size, first,
                                     ents.size - first, _vp(out)), "qh_qpack_dyn_keys")
    return out[:ents.size]


def dyn_keys_dev(codec: HuffmanBatchCodec, entries, nentries, dyn_bytes, nbytes, first, n, keys):
    """qh_dyn_keys_batch over torch tensors in HBM (entries uint8 [>= nentries
    * 32], dyn_bytes uint8, keys uint8 [>= nentries * 16]): keys [first,
    first + n); asynchronous on the codec stream."""
    lib = _load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.qh_dyn_keys_batch(codec._ctx, p(entries), nentries, p(dyn_bytes), nbytes, first, n,
                                     p(keys), _lib.QH_WHERE_DEVICE), "qh_dyn_keys_batch")


def _dyn_index(be, views, nviews, vsel, keys, nentries, max_buckets):
    lib = _load()
    ptr = be.ptr
    recs = be.zeros(max(nviews, 1) * DYN_INDEX_REC_DTYPE.itemsize)
    nsel = 0 if vsel is None else be.size(vsel)

    def call(outs):
        (slots,) = outs
        ns = ctypes.c_uint64(0)
        rv = be.call(lib, "dyn_index", ptr(views), nviews, be.list_ptr(vsel), nsel, ptr(keys), nentries,
                     max_buckets, ptr(recs), ptr(slots), ctypes.byref(ns), be.size(slots) // 4)
        return rv, (int(ns.value),)
    (slots,), (ns,) = be.sized("dyn_index", call, ((4, 1024),), be.empty)
    return recs, slots, ns


def dyn_index(views, keys, vsel=None, max_buckets=0):
    """qh_qpack_dyn_index: the hashed index over the keys (DYN_KEY_DTYPE, the
    whole log's) of views (VIEW_DTYPE) `vsel` (uint32 indices; None: every
    view) -> {"recs": DYN_INDEX_REC_DTYPE [nviews], "slots": uint32,
    "nslots": int}, what the planners take as ``index=``.  `max_buckets`
    (0: no limit) cuts every view's bucket count to a power of two."""
    vw = np.ascontiguousarray(views, dtype=VIEW_DTYPE).reshape(-1)
    ks = np.ascontiguousarray(keys, dtype=DYN_KEY_DTYPE).reshape(-1)
    recs, slots, ns = _dyn_index(Backend(), vw.view(np.uint8), vw.size, _as(vsel, np.uint32),
                                 ks.view(np.uint8), ks.size, max_buckets)
    return {"recs": recs.view(DYN_INDEX_REC_DTYPE)[:vw.size], "slots": slots.view(np.uint32), "nslots": ns}


def dyn_index_dev(codec: HuffmanBatchCodec, views, keys, nentries, vsel=None, max_buckets=0):
    """qh_dyn_index_batch over torch tensors in HBM (views uint8 [nviews *
    40], keys uint8 [>= nentries * 16], vsel int32 or None) -> {"recs" uint8
    [nviews * 48], "slots" uint8 [>= nslots * 4], "nslots"}.  A sizing call
    and the build: each waits once, for the total."""
    be = Backend(views.device, codec)
    recs, slots, ns = _dyn_index(be, views, views.numel() // VIEW_DTYPE.itemsize, vsel, keys, nentries,
                                 max_buckets)
    return {"recs": recs, "slots": slots, "nslots": ns}


def _plan_index(index, d):
    """-> (qh_plan_dyn_index or None, the arrays it points into) from a
    dyn_index / dyn_index_dev result (or any dict of "recs", "slots",
    "nslots": numpy arrays or torch tensors), for the table states d."""
    if index is None or d is None:
        return None, ()
    recs, slots = index["recs"], index["slots"]
    if isinstance(recs, np.ndarray):
        recs = np.ascontiguousarray(recs, dtype=DYN_INDEX_REC_DTYPE).reshape(-1)
        slots = np.ascontiguousarray(slots, dtype=np.uint32).reshape(-1)
        if recs.size < d.nviews or slots.size < index["nslots"]:
            raise ValueError("index smaller than the views or than nslots")
        p = lambda a: a.ctypes.data if a.size else None
    else:
        if recs.numel() < d.nviews * DYN_INDEX_REC_DTYPE.itemsize or slots.numel() < index["nslots"] * 4:
            raise ValueError("index smaller than the views or than nslots")
        p = lambda t: t.data_ptr() if t.numel() else None
    return qh_plan_dyn_index(p(recs), p(slots), int(index["nslots"])), (recs, slots)


def _plan_dyn_host(table, views, section_view, ref_limit, entries, keys, dyn_bytes):
    """-> (qh_plan_dyn or None, the arrays it points into) from host arrays:
    `table` (a DynamicTable: its log, keys and, without `views`, its current
    state) or views / entries / keys / dyn_bytes."""
    if table is not None:
        views = table.view() if views is None else views
        entries, dyn_bytes, keys = table.entries(), table.bytes(), table.keys()
    if views is None:
        if section_view is not None:
            raise ValueError("section_view without views")
        return None, ()
    vw = np.ascontiguousarray(views, dtype=VIEW_DTYPE).reshape(-1)
    sv = _as(section_view, np.uint32)
    rl = _as(ref_limit, np.uint64)
    ents = np.zeros(0, DYN_ENTRY_DTYPE) if entries is None else \
        np.ascontiguousarray(entries, dtype=DYN_ENTRY_DTYPE)
    byts = _u8(b"" if dyn_bytes is None else dyn_bytes)
    ks = dyn_keys(ents, byts) if keys is None else np.ascontiguousarray(keys, dtype=DYN_KEY_DTYPE)
    opt = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    d = qh_plan_dyn(opt(vw), vw.size, opt(sv), opt(rl), opt(ents), ents.size, opt(ks), opt(byts),
                    byts.size)
    return d, (vw, sv, rl, ents, ks, byts)


def _plan_dyn_dev(table, device, views, section_view, ref_limit, entries, keys, dyn_bytes,
                  nentries=None, nbytes=None):
    """The same from torch tensors in HBM (views uint8 [nviews * 40],
    section_view int32, ref_limit int64, entries uint8 [n * 32], keys uint8
    [n * 16], dyn_bytes uint8); `table` is uploaded with to_device."""
    if table is not None:
        d = table.to_device(device)
        views = d["views"] if views is None else views
        entries, keys, dyn_bytes = d["entries"], d["keys"], d["bytes"]
        nentries, nbytes = d["nentries"], d["nbytes"]
    if views is None:
        if section_view is not None:
            raise ValueError("section_view without views")
        return None, ()
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    if nentries is None:
        nentries = 0 if entries is None else entries.numel() // DYN_ENTRY_DTYPE.itemsize
    ne = nentries
    nb = (0 if dyn_bytes is None else dyn_bytes.numel()) if nbytes is None else nbytes
    d = qh_plan_dyn(p(views), views.numel() // VIEW_DTYPE.itemsize, p(section_view), p(ref_limit),
                    p(entries), ne, p(keys), p(dyn_bytes), nb)
    return d, (views, section_view, ref_limit, entries, keys, dyn_bytes)


def plan_fields_dyn(plain, strs, never, field_start, table=None, views=None, section_view=None,
                    ref_limit=None, entries=None, keys=None, dyn_bytes=None, codec=None, index=None):
    """qh_qpack_plan_fields_dyn: the fields (strs[2i], strs[2i+1]) of
    sections [field_start[b], field_start[b+1]) planned against a frozen
    dynamic table (`table`, or views / entries / keys / dyn_bytes; section b
    against views[section_view[b]], referencing entries a + 1 <=
    ref_limit[b]).  -> dict: lines, prefixes (PREFIX_DTYPE), max_cnt, min_cnt.
    With `codec` the same on the GPU over the host arrays
    (qh_plan_fields_dyn_batch, staged).  With `index` (dyn_index's result,
    or a table's ``index()``) the lookups walk its chains instead of
    scanning (qh_qpack_plan_fields_dyn_indexed /
    qh_plan_fields_dyn_indexed_batch): the same result."""
    lib = _load()
    plain = _plain(plain)
    strs = np.ascontiguousarray(strs, dtype=SPAN_IN_DTYPE)
    nf = strs.size // 2
    fs = np.ascontiguousarray(field_start, dtype=np.uint32)
    nsec = fs.size - 1
    nv = _as(never, np.uint8)
    d, keep = _plan_dyn_host(table, views, section_view, ref_limit, entries, keys, dyn_bytes)
    lines = np.zeros(max(nf, 1), dtype=FIELD_LINE_DTYPE)
    pfx = np.zeros(max(nsec, 1), dtype=PREFIX_DTYPE)
    mx = np.zeros(max(nsec, 1), dtype=np.uint64)
    mn = np.zeros(max(nsec, 1), dtype=np.uint64)
    dp = None if d is None else ctypes.byref(d)
    x, xkeep = _plan_index(index, d)
    stem = "plan_fields_dyn" if x is None else "plan_fields_dyn_indexed"
    args = (_vp(plain), _vp(strs), nf, None if nv is None else _vp(nv), _vp(fs), nsec, dp) + \
        (() if x is None else (ctypes.byref(x),)) + (_vp(lines), _vp(pfx), _vp(mx), _vp(mn))
    if codec is None:
        _lib.check(getattr(lib, "qh_qpack_" + stem)(*args), "qh_qpack_" + stem)
    else:
        _lib.check(getattr(lib, "qh_%s_batch" % stem)(codec._ctx, *args, _lib.QH_WHERE_HOST),
                   "qh_%s_batch" % stem)
    del keep, xkeep
    return {"lines": lines[:nf], "prefixes": pfx[:nsec], "max_cnt": mx[:nsec], "min_cnt": mn[:nsec]}


def plan_fields_dyn_dev(codec: HuffmanBatchCodec, plain, strs, never, field_start, lines, prefixes,
                        max_cnt=None, min_cnt=None, table=None, views=None, section_view=None,
                        ref_limit=None, entries=None, keys=None, dyn_bytes=None, nentries=None,
                        nbytes=None, index=None):
    """Device-resident form over torch tensors (plan_fields_dev's, plus
    field_start int32 [nsec + 1], prefixes uint8 [nsec * 24], max_cnt /
    min_cnt int64 [nsec] or None); asynchronous on the codec stream, no host
    wait.  `index`: dyn_index_dev's result, or ``to_device(...)["index"]``
    (qh_plan_fields_dyn_indexed_batch)."""
    lib = _load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    d, keep = _plan_dyn_dev(table, plain.device, views, section_view, ref_limit, entries, keys,
                            dyn_bytes, nentries, nbytes)
    x, xkeep = _plan_index(index, d)
    stem = "qh_plan_fields_dyn_batch" if x is None else "qh_plan_fields_dyn_indexed_batch"
    args = (codec._ctx, p(plain), p(strs), strs.shape[0] // 2, p(never), p(field_start),
            field_start.shape[0] - 1, None if d is None else ctypes.byref(d)) + \
        (() if x is None else (ctypes.byref(x),)) + \
        (p(lines), p(prefixes), p(max_cnt), p(min_cnt), _lib.QH_WHERE_DEVICE)
    _lib.check(getattr(lib, stem)(*args), stem)
    return keep + xkeep


def static_entry(idx: int):
    """qh_qpack_static_entry: (name, value) of static table entry idx."""
    lib = _load()
    n, v = ctypes.c_void_p(), ctypes.c_void_p()
    nl, vl = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.qh_qpack_static_entry(idx, ctypes.byref(n), ctypes.byref(nl), ctypes.byref(v),
                                         ctypes.byref(vl)), "qh_qpack_static_entry")
    return ctypes.string_at(n, nl.value), ctypes.string_at(v, vl.value) if vl.value else b""


def plan_fields(plain, strs, never=None):
    """qh_qpack_plan_fields: fields (strs[2i], strs[2i+1]) of plain -> the
    field lines the reference encoder writes at dynamic table capacity 0."""
    lib = _load()
    plain = _plain(plain)
    strs = np.ascontiguousarray(strs, dtype=SPAN_IN_DTYPE)
    nf = strs.size // 2
    lines = np.zeros(max(nf, 1), dtype=FIELD_LINE_DTYPE)
    nv = _as(never, np.uint8)
    _lib.check(lib.qh_qpack_plan_fields(_vp(plain), _vp(strs), nf, None if nv is None else _vp(nv),
                                        _vp(lines)), "qh_qpack_plan_fields")
    return lines[:nf]


def plan_fields_host(codec: HuffmanBatchCodec, plain, strs, never=None):
    """plan_fields on the GPU over host arrays (qh_plan_fields_batch,
    staged): the same lines, byte for byte."""
    lib = _load()
    plain = _plain(plain)
    strs = np.ascontiguousarray(strs, dtype=SPAN_IN_DTYPE)
    nf = strs.size // 2
    lines = np.zeros(max(nf, 1), dtype=FIELD_LINE_DTYPE)
    nv = _as(never, np.uint8)
    _lib.check(lib.qh_plan_fields_batch(codec._ctx, _vp(plain), _vp(strs), nf,
                                        None if nv is None else _vp(nv), _vp(lines),
                                        _lib.QH_WHERE_HOST), "qh_plan_fields_batch")
    return lines[:nf]


def plan_fields_dev(codec: HuffmanBatchCodec, plain, strs, never, lines):
    """Device-resident form over torch tensors (plain uint8, strs int64
    [2 * nfields, 2] in SPAN_IN layout, never uint8 [nfields] or None, lines
    uint8 [nfields * 24]); asynchronous on the codec stream, no host wait."""
    lib = _load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.qh_plan_fields_batch(codec._ctx, p(plain), p(strs), strs.shape[0] // 2, p(never),
                                        p(lines), _lib.QH_WHERE_DEVICE), "qh_plan_fields_batch")


class FieldSectionEncoder:
    """Whole field sections out of one qh_encode_sections_batch call: the
    count kernels, Huffman iff shorter, the encode kernels over the picked
    strings, then the representation writer kernel (byte for byte
    qh_qpack_write_sections).  ``encode_fields`` / ``encode_fields_dev``
    start from fields instead of planned lines (qh_encode_fields_batch: the
    plan kernel, then the same writer)."""

    def __init__(self, device: int = 0, codec: HuffmanBatchCodec | None = None):
        self.codec = codec or HuffmanBatchCodec(device)

    @staticmethod
    def _with_dst(what, call):
        """call(dst, dst_cap, need) over a dst of 64 bytes, made once more
        with one of the need when that was short -> dst's written bytes."""
        need = ctypes.c_uint64(0)
        dst = np.zeros(64, dtype=np.uint8)
        for _ in range(2):
            rv = call(_vp(dst), dst.size, ctypes.byref(need))
            if rv == _lib.QH_ERR_NOMEM and need.value > dst.size:
                dst = np.zeros(int(need.value), dtype=np.uint8)
                continue
            _lib.check(rv, what)
            break
        return dst[:need.value]

    def encode_sections(self, plain, strs, lines, line_start, prefixes=None):
        """Host arrays -> (dst uint8, sections SPAN_IN_DTYPE)."""
        lib = _load()
        plain = _plain(plain)
        strs = np.ascontiguousarray(strs, dtype=SPAN_IN_DTYPE)
        lines = np.ascontiguousarray(lines, dtype=FIELD_LINE_DTYPE)
        if lines.size == 0:
            lines = np.zeros(1, dtype=FIELD_LINE_DTYPE)[:0]
        line_start = np.ascontiguousarray(line_start, dtype=np.uint32)
        nsec = line_start.size - 1
        pf = _as(prefixes, PREFIX_DTYPE)
        sections = np.zeros(max(nsec, 1), dtype=SPAN_IN_DTYPE)
        dst = self._with_dst("qh_encode_sections_batch", lambda dst, cap, need: lib.qh_encode_sections_batch(
            self.codec._ctx, _vp(plain), _vp(strs), strs.size, _vp(lines), _vp(line_start), nsec,
            None if pf is None else _vp(pf), dst, cap, _vp(sections), need, _lib.QH_WHERE_HOST))
        return dst, sections[:nsec]

    def encode_sections_dev(self, plain, strs, lines, line_start, dst, sections, prefixes=None):
        """Device-resident form over torch tensors (plain uint8, strs int64
        [n,2], lines uint8 [nlines*24], line_start int32 [nsec+1], dst uint8,
        sections int64 [nsec,2], prefixes optional).  Returns dst_need;
        raises on QH_ERR_NOMEM."""
        lib = _load()
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        need = ctypes.c_uint64(0)
        rv = lib.qh_encode_sections_batch(self.codec._ctx, p(plain), p(strs), strs.shape[0], p(lines),
                                          p(line_start), line_start.shape[0] - 1, p(prefixes), p(dst),
                                          dst.numel(), p(sections), ctypes.byref(need),
                                          _lib.QH_WHERE_DEVICE)
        _lib.check(rv, "qh_encode_sections_batch")
        return need.value

    def encode_fields(self, plain, fields, field_start, table=None, views=None, section_view=None,
                      ref_limit=None, entries=None, keys=None, dyn_bytes=None, index=None):
        """Host arrays: fields (FIELD_DTYPE; offsets into plain) of sections
        [field_start[b], field_start[b + 1]) -> (dst uint8, sections
        SPAN_IN_DTYPE), the bytes of write_sections(plan_fields(...)).  With
        `table` (a DynamicTable) or `views` (with entries / keys / dyn_bytes;
        `section_view` / `ref_limit` as plan_fields_dyn takes them) the
        fields are planned against it (qh_encode_fields_dyn_batch) and the
        result is (dst, sections, max_cnt, min_cnt); `index` (dyn_index's
        result) takes the lookups through the hashed index
        (qh_encode_fields_dyn_indexed_batch)."""
        lib = _load()
        if table is not None or views is not None:
            return self._encode_fields_dyn(plain, fields, field_start, table, views, section_view,
                                           ref_limit, entries, keys, dyn_bytes, index)
        plain = _plain(plain)
        fields = np.ascontiguousarray(fields, dtype=FIELD_DTYPE)
        if fields.size == 0:
            fields = np.zeros(1, dtype=FIELD_DTYPE)[:0]
        field_start = np.ascontiguousarray(field_start, dtype=np.uint32)
        nsec = field_start.size - 1
        sections = np.zeros(max(nsec, 1), dtype=SPAN_IN_DTYPE)
        dst = self._with_dst("qh_encode_fields_batch", lambda dst, cap, need: lib.qh_encode_fields_batch(
            self.codec._ctx, _vp(plain), _vp(fields), fields.size, _vp(field_start), nsec, dst, cap,
            _vp(sections), need, _lib.QH_WHERE_HOST))
        return dst, sections[:nsec]

    def _encode_fields_dyn(self, plain, fields, field_start, table, views, section_view, ref_limit,
                           entries, keys, dyn_bytes, index=None):
        lib = _load()
        plain = _plain(plain)
        fields = np.ascontiguousarray(fields, dtype=FIELD_DTYPE)
        if fields.size == 0:
            fields = np.zeros(1, dtype=FIELD_DTYPE)[:0]
        field_start = np.ascontiguousarray(field_start, dtype=np.uint32)
        nsec = field_start.size - 1
        d, keep = _plan_dyn_host(table, views, section_view, ref_limit, entries, keys, dyn_bytes)
        sections = np.zeros(max(nsec, 1), dtype=SPAN_IN_DTYPE)
        mx = np.zeros(max(nsec, 1), dtype=np.uint64)
        mn = np.zeros(max(nsec, 1), dtype=np.uint64)
        x, xkeep = _plan_index(index, d)
        stem = "qh_encode_fields_dyn_batch" if x is None else "qh_encode_fields_dyn_indexed_batch"
        fn = getattr(lib, stem)
        dst = self._with_dst(stem, lambda dst, cap, need: fn(
            self.codec._ctx, _vp(plain), _vp(fields), fields.size, _vp(field_start), nsec,
            None if d is None else ctypes.byref(d), *(() if x is None else (ctypes.byref(x),)), dst, cap,
            _vp(sections), need, _vp(mx), _vp(mn), _lib.QH_WHERE_HOST))
        del keep, xkeep
        return dst, sections[:nsec], mx[:nsec], mn[:nsec]

    def encode_fields_dev(self, plain, fields, nfields, field_start, dst, sections, table=None,
                          views=None, section_view=None, ref_limit=None, max_cnt=None, min_cnt=None,
                          entries=None, keys=None, dyn_bytes=None, nentries=None, nbytes=None,
                          index=None):
        """Device-resident form over torch tensors, emit_fields_dev's as they
        are: plain uint8 (its `out`), fields uint8 [>= nfields * 32],
        field_start int32 [nsec + 1], dst uint8, sections int64 [nsec, 2].
        Returns dst_need; raises on QH_ERR_NOMEM.  With `table` (uploaded
        with to_device) or views / entries / keys / dyn_bytes tensors the
        fields are planned against the table (qh_encode_fields_dyn_batch);
        max_cnt / min_cnt (int64 [nsec]) then receive every section's
        reference counts, and the result is (dst_need, max_cnt, min_cnt);
        `index` (dyn_index_dev's result) takes the lookups through the
        hashed index (qh_encode_fields_dyn_indexed_batch)."""
        lib = _load()
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        need = ctypes.c_uint64(0)
        if table is not None or views is not None:
            import torch
            nsec = field_start.shape[0] - 1
            d, keep = _plan_dyn_dev(table, plain.device, views, section_view, ref_limit, entries,
                                    keys, dyn_bytes, nentries, nbytes)
            if max_cnt is None:
                max_cnt = torch.empty(max(nsec, 1), dtype=torch.int64, device=plain.device)
            if min_cnt is None:
                min_cnt = torch.empty(max(nsec, 1), dtype=torch.int64, device=plain.device)
            x, xkeep = _plan_index(index, d)
            stem = "qh_encode_fields_dyn_batch" if x is None else "qh_encode_fields_dyn_indexed_batch"
            rv = getattr(lib, stem)(self.codec._ctx, p(plain), p(fields), int(nfields), p(field_start), nsec,
                                    ctypes.byref(d), *(() if x is None else (ctypes.byref(x),)), p(dst),
                                    dst.numel(), p(sections), ctypes.byref(need), p(max_cnt), p(min_cnt),
                                    _lib.QH_WHERE_DEVICE)
            _lib.check(rv, stem)
            del keep, xkeep  # (the call has waited for the totals)
            return need.value, max_cnt, min_cnt
        rv = lib.qh_encode_fields_batch(self.codec._ctx, p(plain), p(fields), int(nfields),
                                        p(field_start), field_start.shape[0] - 1, p(dst), dst.numel(),
                                        p(sections), ctypes.byref(need), _lib.QH_WHERE_DEVICE)
        _lib.check(rv, "qh_encode_fields_batch")
        return need.value
