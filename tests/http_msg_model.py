"""A Python restatement of the reference's HTTP message checks, the judge of
qh_qpack_http_check: lib/nghttp3_http.c:62-122 (parse_status_code, parse_uint,
check_pseudo_header, expect_response_body, check_path_flags), :208-317 (the
value checks), :319-627 (the two on_header switches, nghttp3_http_on_header,
the two end-of-headers functions), :715-727 and :798-838 (the name and value
checks), walked as conn_decode_headers walks a section
(lib/nghttp3_conn.c:1880-1944, :1713-1730).  Written from the reference,
function by function, and driven by the reference's own class tables
(tests/golden/http_chars.json, tests/golden/http_msg_chars.json); the C core
uses range compares instead.  The `priority` dictionary is not parsed (the
library's stated departure: :437-449 are left out), and a section that ends
malformed gives back the state it was given (the second departure).  The
model is itself held against the reference library's transcripts on every
case in tests/test_http_ref.py."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_A = json.load(open(os.path.join(GOLDEN, "http_chars.json")))
_B = json.load(open(os.path.join(GOLDEN, "http_msg_chars.json")))
NAME_CHARS = _A["VALID_HD_NAME_CHARS"]
VALUE_CHARS = _A["VALID_HD_VALUE_CHARS"]
WS = set(_A["is_ws"])
AUTHORITY_CHARS = _B["VALID_AUTHORITY_CHARS"]
METHOD_CHARS = _B["VALID_METHOD_CHARS"]
PATH_CHARS = _B["VALID_PATH_CHARS"]
TOKENS = json.load(open(os.path.join(GOLDEN, "tokens.json")))["tokens"]

MALFORMED, REMOVE = -105, -106  # NGHTTP3_ERR_MALFORMED_HTTP_HEADER, _REMOVE_HTTP_HEADER
KEEP_V, REMOVE_V, MALFORMED_V, UNSEEN_V = 0, 1, 2, 3
REQUEST, TRAILERS, CONNECT_PROTOCOL = 1, 2, 4
NO_FIELD = 0xFFFFFFFF

# lib/nghttp3_http.h:42-83
F_AUTHORITY, F_PATH, F_METHOD, F_SCHEME, F_HOST, F_STATUS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
F_REQ_HEADERS = F_METHOD | F_PATH | F_SCHEME
F_PSEUDO_HEADER_DISALLOWED = 0x40
F_METH_CONNECT, F_METH_HEAD, F_METH_OPTIONS = 0x80, 0x100, 0x200
F_METH_ALL = F_METH_CONNECT | F_METH_HEAD | F_METH_OPTIONS
F_PATH_REGULAR, F_PATH_ASTERISK, F_SCHEME_HTTP = 0x400, 0x800, 0x1000
F_EXPECT_FINAL_RESPONSE, F_PROTOCOL, F_PRIORITY, F_BAD_PRIORITY = 0x2000, 0x4000, 0x8000, 0x10000
MAX_VARINT = (1 << 62) - 1


def token_of(name: bytes) -> int:
    try:
        return TOKENS.get(name.decode("ascii"), -1)
    except UnicodeDecodeError:
        return -1


class State:
    def __init__(self, content_length=-1, status_code=-1, flags=0):
        self.content_length, self.status_code, self.flags = content_length, status_code, flags

    def copy(self):
        return State(self.content_length, self.status_code, self.flags)

    def tuple(self):
        return (self.content_length, self.status_code, self.flags)


def cdiv100(x):  # C's division truncates towards zero: -1 / 100 == 0
    return int(x / 100)


def parse_status_code(s):
    if len(s) != 3 or not (0x31 <= s[0] <= 0x39) or not (0x30 <= s[1] <= 0x39) or \
            not (0x30 <= s[2] <= 0x39):
        return -1
    return (s[0] - 0x30) * 100 + (s[1] - 0x30) * 10 + (s[2] - 0x30)


def parse_uint(s):
    if len(s) == 0:
        return -1
    n = 0
    for b in s:
        if b < 0x30 or b > 0x39:
            return -1
        c = b - 0x30
        if n > (MAX_VARINT - c) // 10:
            return -1
        n = n * 10 + c
    return n


def check_pseudo_header(http, value, flag):
    if (http.flags & flag) or len(value) == 0:
        return False
    http.flags |= flag
    return True


def expect_response_body(http):
    return (http.flags & F_METH_HEAD) == 0 and cdiv100(http.status_code) != 1 and \
        http.status_code != 304 and http.status_code != 204


def check_path_flags(http):
    return (http.flags & F_SCHEME_HTTP) == 0 or bool(
        (http.flags & F_PATH_REGULAR) or ((http.flags & F_METH_OPTIONS) and (http.flags & F_PATH_ASTERISK)))


def check_authority(v):
    return all(AUTHORITY_CHARS[b] for b in v)


def check_scheme(v):
    if len(v) == 0:
        return False
    alpha = lambda b: 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A
    if not alpha(v[0]):
        return False
    return all(alpha(b) or 0x30 <= b <= 0x39 or b in b"+-." for b in v[1:])


def check_method(v):
    return len(v) != 0 and all(METHOD_CHARS[b] for b in v)


def check_path(v):
    return all(PATH_CHARS[b] for b in v)


def check_header_value(v):
    if len(v) == 0:
        return True
    if v[0] in WS or v[-1] in WS:
        return False
    return all(VALUE_CHARS[b] for b in v)


def check_nonempty_header_name(name):
    for b in name:
        if NAME_CHARS[b] != 1:
            return NAME_CHARS[b]
    return 1


def lstrieq(lit, v):
    return len(lit) == len(v) and bytes(v).lower() == lit


def T(name):
    return TOKENS[name]


DISALLOWED = {T("connection"), T("keep-alive"), T("proxy-connection"), T("transfer-encoding"), T("upgrade")}


def request_on_header(http, name, value, token, trailers, connect_protocol):
    if token == T(":authority"):
        if not check_authority(value) or not check_pseudo_header(http, value, F_AUTHORITY):
            return MALFORMED
    elif token == T(":method"):
        if not check_method(value) or not check_pseudo_header(http, value, F_METHOD):
            return MALFORMED
        if value == b"HEAD":
            http.flags |= F_METH_HEAD
        elif value == b"CONNECT":
            http.flags |= F_METH_CONNECT
        elif value == b"OPTIONS":
            http.flags |= F_METH_OPTIONS
    elif token == T(":path"):
        if not check_path(value) or not check_pseudo_header(http, value, F_PATH):
            return MALFORMED
        if value[0] == 0x2F:
            http.flags |= F_PATH_REGULAR
        elif value == b"*":
            http.flags |= F_PATH_ASTERISK
    elif token == T(":scheme"):
        if not check_scheme(value) or not check_pseudo_header(http, value, F_SCHEME):
            return MALFORMED
        if lstrieq(b"http", value) or lstrieq(b"https", value):
            http.flags |= F_SCHEME_HTTP
    elif token == T(":protocol"):
        if not connect_protocol or not check_header_value(value) or \
                not check_pseudo_header(http, value, F_PROTOCOL):
            return MALFORMED
    elif token == T("host"):
        if not check_authority(value):
            return REMOVE
        if not check_pseudo_header(http, value, F_HOST):
            return MALFORMED
    elif token == T("content-length"):
        if trailers:
            return REMOVE
        if http.content_length != -1:
            return MALFORMED
        http.content_length = parse_uint(value)
        if http.content_length == -1:
            return MALFORMED
    elif token in DISALLOWED:
        return MALFORMED
    elif token == T("te"):
        if not lstrieq(b"trailers", value):
            return MALFORMED
    elif token == T("priority"):
        if not check_header_value(value):
            http.flags &= ~F_PRIORITY
            http.flags |= F_BAD_PRIORITY
            return REMOVE
        # (the dictionary parse, :433-449, is the library's departure: kept as it is)
    else:
        if name[0] == 0x3A:
            return MALFORMED
        if not check_header_value(value):
            return REMOVE
    return 0


def response_on_header(http, name, value, token, trailers):
    if token == T(":status"):
        if not check_pseudo_header(http, value, F_STATUS):
            return MALFORMED
        http.status_code = parse_status_code(value)
        if http.status_code == -1 or http.status_code == 101:
            return MALFORMED
    elif token == T("content-length"):
        if trailers:
            return REMOVE
        if http.status_code == 204:
            if http.content_length != -1 or not lstrieq(b"0", value):
                return MALFORMED
            http.content_length = 0
            return REMOVE
        if cdiv100(http.status_code) == 1 or \
                (cdiv100(http.status_code) == 2 and (http.flags & F_METH_CONNECT)):
            return REMOVE
        if http.content_length != -1:
            return MALFORMED
        http.content_length = parse_uint(value)
        if http.content_length == -1:
            return MALFORMED
    elif token in DISALLOWED:
        return MALFORMED
    elif token == T("te"):
        if not lstrieq(b"trailers", value):
            return MALFORMED
    else:
        if name[0] == 0x3A:
            return MALFORMED
        if not check_header_value(value):
            return REMOVE
    return 0


def on_header(http, name, value, token, request, trailers, connect_protocol):
    if len(name) == 0:
        http.flags |= F_PSEUDO_HEADER_DISALLOWED
        return REMOVE
    if name[0] == 0x3A:
        if token == -1 or trailers or (http.flags & F_PSEUDO_HEADER_DISALLOWED):
            return MALFORMED
    else:
        http.flags |= F_PSEUDO_HEADER_DISALLOWED
        rv = check_nonempty_header_name(name)
        if rv == 0:
            return REMOVE
        if rv == -1:
            return MALFORMED
    if request:
        return request_on_header(http, name, value, token, trailers, connect_protocol)
    return response_on_header(http, name, value, token, trailers)


def on_request_headers(http):
    if not (http.flags & F_PROTOCOL) and (http.flags & F_METH_CONNECT):
        if (http.flags & (F_SCHEME | F_PATH)) or (http.flags & F_AUTHORITY) == 0:
            return MALFORMED
        http.content_length = -1
    else:
        if (http.flags & F_REQ_HEADERS) != F_REQ_HEADERS or (http.flags & (F_AUTHORITY | F_HOST)) == 0:
            return MALFORMED
        if http.flags & F_PROTOCOL:
            if (http.flags & F_METH_CONNECT) == 0 or (http.flags & F_AUTHORITY) == 0:
                return MALFORMED
            http.content_length = -1
        if not check_path_flags(http):
            return MALFORMED
    return 0


def on_response_headers(http):
    if (http.flags & F_STATUS) == 0:
        return MALFORMED
    if cdiv100(http.status_code) == 1:
        http.flags = (http.flags & F_METH_ALL) | F_EXPECT_FINAL_RESPONSE
        http.content_length = -1
        http.status_code = -1
        return 0
    http.flags &= ~F_EXPECT_FINAL_RESPONSE
    if not expect_response_body(http):
        http.content_length = 0
    elif http.flags & F_METH_CONNECT:
        http.content_length = -1
    return 0


def section(fields, kind, state):
    """One section as conn_decode_headers and the end of its headers treat it.
    fields: (name, value, token) each.  -> (verdicts, status, bad_field, kept
    indices, the state afterwards)."""
    http = state.copy()
    request, trailers = bool(kind & REQUEST), bool(kind & TRAILERS)
    verdicts = [UNSEEN_V] * len(fields)
    kept = []
    for i, (name, value, token) in enumerate(fields):
        rv = on_header(http, name, value, token, request, trailers, bool(kind & CONNECT_PROTOCOL))
        if rv == MALFORMED:
            verdicts[i] = MALFORMED_V
            return verdicts, MALFORMED, i, kept, state.copy()
        verdicts[i] = REMOVE_V if rv == REMOVE else KEEP_V
        if rv == 0:
            kept.append(i)
    rv = 0
    if not trailers:
        rv = on_request_headers(http) if request else on_response_headers(http)
    if rv != 0:
        return verdicts, MALFORMED, len(fields), kept, state.copy()
    return verdicts, 0, NO_FIELD, kept, http
