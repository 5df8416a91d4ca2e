/*
 * qhuff.h -- C ABI of the MI355X QPACK Huffman engine (libqhuff.so).
 *
 * Two families of entry points:
 *
 * 1. Exact-signature drop-ins for nghttp3's private Huffman codec
 *    (lib/nghttp3_qpack_huffman.h:42-107; implementation
 *    lib/nghttp3_qpack_huffman.c:34-129; data
 *    lib/nghttp3_qpack_huffman_data.c:30-96,98-4982).  They keep the
 *    reference names, argument meaning and error behaviour so that
 *    lib/nghttp3_qpack.c links against libqhuff instead of
 *    nghttp3_qpack_huffman.o / nghttp3_qpack_huffman_data.o (the symbols are
 *    hidden inside libnghttp3, so the replacement is at link time; see
 *    INTEGRATION.md).  These serve the streaming case the reference decoder
 *    has: a Huffman string split across nghttp3_qpack_decoder_read_request
 *    calls (qpack.c:2737-2763, fin = 0 until the last chunk).  They run on
 *    the host: a partial chunk of a few bytes cannot amortise a launch.
 *
 * 2. The batch API (qh_*): whole strings gathered by the QPACK layer
 *    (qpack.c call sites :1861,1882,1953,1961,1980,1993 for encode,
 *    :2750,2756 reached from :2992,3083,3606,3694 for decode) are encoded or
 *    decoded by HIP kernels on gfx950.  There is no host fallback: without a
 *    usable HIP device every batch entry point returns QH_ERR_FATAL.
 *
 * Plain C types only; no torch or HIP types appear in any signature
 * (streams are passed as `void *` = hipStream_t).
 */
#ifndef QHUFF_H
#define QHUFF_H

#include <stddef.h>
#include <stdint.h>

#if defined(_WIN32)
#define QH_EXPORT
#else
#define QH_EXPORT __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* 1. Exact-signature drop-ins (reference: lib/nghttp3_qpack_huffman.h)      */
/* ------------------------------------------------------------------------ */

/* nghttp3.h:82 */
typedef ptrdiff_t nghttp3_ssize;

#ifndef NGHTTP3_QPACK_HUFFMAN_H
/* huffman.h:35-40 -- code is MSB-aligned in 32 bits. */
typedef struct nghttp3_qpack_huffman_sym {
  uint32_t nbits;
  uint32_t code;
} nghttp3_qpack_huffman_sym;

/* huffman.h:51,54 */
#define NGHTTP3_QPACK_HUFFMAN_FLAG_ACCEPTED 0x01U
#define NGHTTP3_QPACK_HUFFMAN_FLAG_SYM 0x02U

/* huffman.h:56-68 */
typedef struct nghttp3_qpack_huffman_decode_node {
  uint16_t fstate;
  uint8_t flags;
  uint8_t sym;
} nghttp3_qpack_huffman_decode_node;

/* huffman.h:70-74 */
typedef struct nghttp3_qpack_huffman_decode_context {
  uint16_t fstate;
  uint8_t flags;
} nghttp3_qpack_huffman_decode_context;

/* huffman.h:113-115 */
static inline size_t nghttp3_qpack_huffman_estimate_decode_length(size_t len) {
  return len * 8 / 5;
}
#endif /* !NGHTTP3_QPACK_HUFFMAN_H */

/* huffman.h:42 / huffman_data.c:30-96 */
QH_EXPORT extern const nghttp3_qpack_huffman_sym huffman_sym_table[];
/* huffman.h:76 / huffman_data.c:98-4982 */
QH_EXPORT extern const nghttp3_qpack_huffman_decode_node
    qpack_huffman_decode_table[][16];

/* huffman.h:44 (huffman.c:34-43): ceil(sum of code lengths / 8). */
QH_EXPORT size_t nghttp3_qpack_huffman_encode_count(const uint8_t *src,
                                                    size_t len);
/* huffman.h:46-47 (huffman.c:45-78): writes exactly encode_count bytes,
 * returns dest + that count. */
QH_EXPORT uint8_t *nghttp3_qpack_huffman_encode(uint8_t *dest,
                                                const uint8_t *src,
                                                size_t srclen);
/* huffman.h:78-79 (huffman.c:80-85) */
QH_EXPORT void nghttp3_qpack_huffman_decode_context_init(
    nghttp3_qpack_huffman_decode_context *ctx);
/* huffman.h:97-100 (huffman.c:87-124): bytes written, or -108
 * (NGHTTP3_ERR_QPACK_FATAL) when fin && the final state is not accepting. */
QH_EXPORT nghttp3_ssize nghttp3_qpack_huffman_decode(
    nghttp3_qpack_huffman_decode_context *ctx, uint8_t *dest,
    const uint8_t *src, size_t srclen, int fin);
/* huffman.h:106-107 (huffman.c:126-129) */
QH_EXPORT int nghttp3_qpack_huffman_decode_failure_state(
    const nghttp3_qpack_huffman_decode_context *ctx);

/* ------------------------------------------------------------------------ */
/* 2. Batch API (HIP, gfx950)                                                */
/* ------------------------------------------------------------------------ */

/* Return codes (values follow lib/includes/nghttp3/nghttp3.h). */
#define QH_OK 0
#define QH_ERR_INVALID_ARGUMENT (-101) /* NGHTTP3_ERR_INVALID_ARGUMENT */
#define QH_ERR_QPACK_FATAL (-108)      /* NGHTTP3_ERR_QPACK_FATAL      */
#define QH_ERR_FATAL (-900)            /* NGHTTP3_ERR_FATAL: HIP failure */
#define QH_ERR_NOMEM (-901)            /* NGHTTP3_ERR_NOMEM            */

/* Where the pointers handed to a batch call live. */
#define QH_WHERE_HOST 0   /* host memory; the call copies H2D/D2H, blocks */
#define QH_WHERE_DEVICE 1 /* HBM; the call is asynchronous on ctx stream */
/* qh_decode_batch only: HBM, asynchronous, the decoded strings packed back
 * to back in dst as with QH_WHERE_HOST (out[i].off = the decoded bytes
 * before string i); the strings are decoded into a context scratch buffer of
 * dst_cap bytes first, then packed (one more pass over the decoded bytes). */
#define QH_WHERE_DEVICE_DENSE 2

/* One string: bytes [off, off + len) of the batch's source buffer. */
typedef struct qh_span_in {
  uint64_t off;
  uint32_t len;
  uint32_t flags; /* QH_SPAN_* bits as written by the QPACK scanners below;
                     ignored by the Huffman batch calls */
} qh_span_in;

/* One result string: bytes [off, off + len) of the batch's destination
 * buffer.  status is 0, QH_ERR_QPACK_FATAL (invalid Huffman string, same
 * verdict as nghttp3_qpack_huffman_decode(..., fin = 1) plus the
 * failure-state check at qpack.c:2756), or QH_ERR_NOMEM (the string's slot
 * does not fit in dst_cap; nothing written). */
typedef struct qh_span_out {
  uint64_t off;
  uint32_t len;
  int32_t status;
} qh_span_out;

/* Totals of the most recent batch call on a context. */
typedef struct qh_batch_stats {
  uint64_t n;          /* strings                                    */
  uint64_t in_bytes;   /* sum of input lengths                       */
  uint64_t out_bytes;  /* sum of output lengths (successful strings) */
  uint64_t dst_bytes;  /* destination bytes the layout occupies      */
  uint64_t n_errors;   /* strings with status != 0                   */
  /* decode with QH_DECODER_WINDOWS / _SORTED: lock-step iterations (16
   * table lookups each) run by lanes, and by waves (each wave counts its
   * longest lane per window); lane_steps / (64 * wave_steps) is the active-
   * lane fraction.  Counted only by the instrumented development build
   * (make stamps: the counter slows the decoder); 0 otherwise. */
  uint64_t lane_steps;
  uint64_t wave_steps;
} qh_batch_stats;

typedef struct qh_ctx qh_ctx;

/* Bind a context to HIP device `device` and stream `stream` (a hipStream_t;
 * NULL = the device's default stream, as in other HIP libraries).  Every
 * batch call is ordered on that stream. */
QH_EXPORT int qh_ctx_new(qh_ctx **pctx, int device, void *stream);
QH_EXPORT void qh_ctx_del(qh_ctx *ctx);
QH_EXPORT int qh_ctx_set_stream(qh_ctx *ctx, void *stream);
/* Decoder kernel of qh_decode_batch (results are identical; speed is not):
 * QH_DECODER_WINDOWS (default) sorts each 256-string window by length and
 * decodes a window per workgroup -- fastest for header strings of similar
 * length (8-256 B, and the 1-128 B strings of whole field sections);
 * QH_DECODER_WAVES lets every wave sort and decode its own chunks of 256
 * strings with no workgroup barrier, its input staged through LDS in
 * 64-byte groups. */
#define QH_DECODER_WINDOWS 0
#define QH_DECODER_WAVES 1
/* QH_DECODER_SORTED: the window decoder over a batch-wide schedule --
 * three short passes over the spans sort the strings into 16-byte length
 * classes, longest first, so every 256-string window holds strings of one
 * class (same output layout).  For skewed lengths and binary text: on one
 * MI355X, Zipf lengths to 4 KiB decode 2.3x the wave decoder and 6x the
 * window decoder, binary text 1.3x; 8-256 B headers ~5% slower than
 * QH_DECODER_WINDOWS (the schedule's ~25 us). */
#define QH_DECODER_SORTED 2
QH_EXPORT int qh_ctx_set_decoder(qh_ctx *ctx, int kind);
/* Codes kernel of qh_encode_batch (results are identical; speed is not):
 * QH_ENCODER_AUTO (default) runs one of the two below per batch, chosen
 * from the strings of the context's previous encode (their lengths' spread
 * and mean, their encoded size; the first encode of a context uses the
 * window encoder): QH_ENCODER_FUSED for skewed, long or binary strings,
 * else QH_ENCODER_WINDOWS.
 * QH_ENCODER_WINDOWS encodes a sorted window of up to 256 strings
 * per workgroup into an LDS stage copied out with coalesced stores --
 * fastest for strings of similar length; QH_ENCODER_WAVES lets every wave
 * sort and encode its own chunks of 256 strings with no workgroup barrier,
 * each lane writing its string's 16-byte output chunks from an LDS ring --
 * fastest for skewed or long strings (Zipf up to 4 KiB: 2.3x). */
#define QH_ENCODER_WINDOWS 0
#define QH_ENCODER_WAVES 1
/* QH_ENCODER_FUSED: one pass over the plaintext -- every lane takes 16 bytes
 * of one string, whatever the string lengths; code bits are summed per
 * string, a decoupled look-back over 4 KiB tiles places each tile in the dense
 * output, and the codes go out through an LDS stage. */
#define QH_ENCODER_FUSED 2
#define QH_ENCODER_AUTO 3
/* QH_ENCODER_REGION: the length pass, then a codes pass that streams the
 * plaintext region of every 64 strings lying back to back in memory (lane j
 * of a wave: bytes [64 j, 64 j + 64) of each 4 KiB round, codes placed by a
 * prefix sum of their lengths and the strings' pads); strings in any other
 * layout a lane each.  Opt-in: QH_ENCODER_AUTO never chooses it. */
#define QH_ENCODER_REGION 4
QH_EXPORT int qh_ctx_set_encoder(qh_ctx *ctx, int kind);
/* Tuning options (results are identical; speed is not).  The library reads
 * no environment variable that changes what it computes or which kernels
 * run: these are set explicitly, per context.
 * QH_OPT_LONG_MIN: QH_DECODER_SORTED decodes strings of at least `value`
 *   encoded bytes (their 16-byte length class and longer) with a workgroup
 *   per string; 0 turns that path off (default 4096; at most 2^30).
 * QH_OPT_LENS_LANE_PASS: 1 counts every string's encoded length a lane per
 *   string (the path the length kernel takes for scattered spans) instead
 *   of streaming the strings' region; 0 (default) chooses per window.
 * QH_OPT_SECTIONS_SLICE_BLOCKS: header blocks per slice of the pipelined
 *   host-memory qh_decode_sections_batch (QH_SECTIONS_PACKED); 0 (default)
 *   lets the library choose.  Any value gives the same results.
 * QH_OPT_EMIT_LONG_MIN: qh_emit_fields_batch copies a name or value of at
 *   least `value` bytes with a wave instead of a lane; 0 (default) lets the
 *   library choose (else 16 .. 2^30).
 * QH_OPT_H3W_LONG_MIN: qh_h3_write_batch copies a payload of at least `value`
 *   bytes with waves, cut into pieces, instead of a 16-lane group; 0 (default)
 *   lets the library choose (else 16 .. 2^30).
 * QH_OPT_H3W_PIECE: the most bytes of such a payload that one wave copies; 0
 *   (default) lets the library choose (else 1024 .. 2^30).
 * No reference counterpart (the reference codec has no batch kernels). */
#define QH_OPT_LONG_MIN 1
#define QH_OPT_LENS_LANE_PASS 2
#define QH_OPT_SECTIONS_SLICE_BLOCKS 3
#define QH_OPT_EMIT_LONG_MIN 4
#define QH_OPT_H3W_LONG_MIN 5
#define QH_OPT_H3W_PIECE 6
QH_EXPORT int qh_ctx_set_option(qh_ctx *ctx, int option, int64_t value);
QH_EXPORT void *qh_ctx_stream(qh_ctx *ctx);
/* Wait for all work queued on the context's stream. */
QH_EXPORT int qh_ctx_sync(qh_ctx *ctx);
/* Totals of the last batch call (synchronises the stream). */
QH_EXPORT int qh_ctx_last_stats(qh_ctx *ctx, qh_batch_stats *stats);

/* Destination sizing.  A decoded string never exceeds the reference's
 * estimate_decode_length(len) = len * 8 / 5 (huffman.h:113-115; the caller
 * of the reference sizes its rcbuf from it, qpack.c:2977,3065,3591,3677).
 * Batch decode gives string i a slot of round_up(len_i * 8 / 5 + 16, 64)
 * bytes, slots in string order and back to back (so every slot starts
 * 64-byte aligned relative to dst), so qh_decode_dst_size(in, n) = the sum
 * of the slots is what a batch needs; out[i].off is the start of the slot
 * and out[i].len the decoded length.  The other bytes of a slot are
 * unspecified.  A string whose slot does not fit in dst_cap gets
 * QH_ERR_NOMEM; nothing is written at or past dst_cap.  With QH_WHERE_HOST
 * the decoded strings come back packed: dst holds them back to back and
 * out[i].off = the sum of the decoded lengths before string i (only decoded
 * bytes cross PCIe; the batch is pipelined in slices over copy and compute
 * streams); dst_cap >= qh_decode_dst_size(in, n) still always suffices, and a
 * string whose bytes would pass dst_cap gets QH_ERR_NOMEM.
 * Encode output is dense: out[i].off = sum_{j<i} encode_count(string j);
 * qh_encode_dst_bound() is an upper bound. */
QH_EXPORT uint64_t qh_decode_dst_size(const qh_span_in *in, size_t n);
QH_EXPORT uint64_t qh_encode_dst_bound(const qh_span_in *in, size_t n);

/* Decode n complete Huffman strings (fin = 1 each). */
QH_EXPORT int qh_decode_batch(qh_ctx *ctx, const uint8_t *src,
                              const qh_span_in *in, size_t n, uint8_t *dst,
                              uint64_t dst_cap, qh_span_out *out, int where);

/* One host-memory batch (as qh_decode_batch with QH_WHERE_HOST) fanned out
 * over n_ctx contexts -- one per GPU, or several on one GPU with their own
 * streams: the strings are cut into n_ctx ranges of about equal encoded
 * bytes, in string order, and context k decodes range k from its own host
 * thread through its own H2D / decode / D2H pipeline (SURVEY.md section
 * 8(e): each GPU receives its shard by its own H2D; the reference has no
 * parallel path).  Range k's decoded strings are packed back to back from
 * dst + B_k, B_k = the sum of len * 8 / 5 (the reference's
 * estimate_decode_length, huffman.h:113-115) over the strings of the ranges
 * before it, so the strings are in global order with a gap between ranges
 * that never exceeds that estimate's slack; out[i].off is the offset in dst.
 * dst_cap >= qh_decode_dst_size(in, n) suffices.  Blocks until every range
 * is done; returns 0 or the first range's error. */
QH_EXPORT int qh_decode_batch_multi(qh_ctx *const *ctxs, int n_ctx, const uint8_t *src,
                                    const qh_span_in *in, size_t n, uint8_t *dst,
                                    uint64_t dst_cap, qh_span_out *out);

/* hlen[i] = nghttp3_qpack_huffman_encode_count(string i). */
QH_EXPORT int qh_encode_count_batch(qh_ctx *ctx, const uint8_t *src,
                                    const qh_span_in *in, size_t n,
                                    uint32_t *hlen, int where);

/* Huffman-encode n strings densely into dst (byte-identical to
 * nghttp3_qpack_huffman_encode per string). */
QH_EXPORT int qh_encode_batch(qh_ctx *ctx, const uint8_t *src,
                              const qh_span_in *in, size_t n, uint8_t *dst,
                              uint64_t dst_cap, qh_span_out *out, int where);

/* Per-kernel HIP-event timing of batch calls (off by default).  When on,
 * every kernel launch is bracketed by events on the context stream;
 * qh_ctx_kernel_times() synchronises and returns, for up to `cap` kernels,
 * their names, launch counts and summed milliseconds, then resets. */
QH_EXPORT int qh_ctx_enable_timing(qh_ctx *ctx, int on);
QH_EXPORT int qh_ctx_kernel_times(qh_ctx *ctx, const char **names,
                                  uint64_t *counts, double *ms, int cap);

/* Deterministic synthetic workloads generated on the device (bench/tests):
 * string i has length lo + splitmix64-draw % (hi - lo + 1) (dist 0, uniform)
 * or a Zipf(s)-distributed length in [lo, hi] (dist 1); strings are packed
 * back to back (in[i].off = prefix sum of lengths) and byte k of the packed
 * buffer is alphabet[draw(k) % alphabet_len].  See nghttp3_amd/synth.py for
 * the bit-exact host restatement. */
QH_EXPORT int qh_synth_spans(qh_ctx *ctx, uint64_t seed, size_t n, uint32_t lo,
                             uint32_t hi, int dist, double zipf_s,
                             qh_span_in *in_dev, uint64_t *total_dev);
/* dst_dev[j] = byte first + j of that packed buffer (a rank generates its
 * own shard of a batch). */
QH_EXPORT int qh_synth_fill(qh_ctx *ctx, uint64_t seed, uint64_t first,
                            uint8_t *dst_dev, uint64_t nbytes,
                            const uint8_t *alphabet, uint32_t alphabet_len);

/* ---- QPACK field-line framing ---------
 * Host C (nghttp3_amd/csrc/qh_qpack.c).  The scanners turn whole encoded
 * field sections (request-stream header blocks) and encoder-stream bytes
 * into field lines plus (off, len, flags) string spans, ready for
 * qh_decode_batch (pass only the spans with QH_SPAN_HUFFMAN; the others are
 * raw octets).  Indices are returned as encoded (static, base-relative or
 * post-base); qh_qpack_emit_fields / qh_emit_fields_batch below resolve them
 * against the static table and a dynamic table state.
 * Replaces the framing of nghttp3_qpack_decoder_read_request
 * (lib/nghttp3_qpack.c:3347-3800) and nghttp3_qpack_decoder_read_encoder
 * (:2815-3150) around the per-string Huffman calls (:2737-2763). */
#define QH_ERR_QPACK_HEADER_TOO_LARGE (-109)     /* nghttp3.h:224 */
#define QH_ERR_QPACK_DECOMPRESSION_FAILED (-401) /* nghttp3.h:252 */
#define QH_ERR_QPACK_ENCODER_STREAM_ERROR (-402) /* nghttp3.h:259 */

#define QH_SPAN_HUFFMAN 0x1u /* H bit set: Huffman-coded string       */
#define QH_SPAN_NAME 0x2u    /* the string is a field name (else value) */

/* Field-line opcodes (qpack.c:3439-3495) and encoder-stream instructions
 * (qpack.c:2837-2875). */
#define QH_FL_INDEXED 1         /* 1Txxxxxx                           */
#define QH_FL_INDEXED_PB 2      /* 0001xxxx  post-base index           */
#define QH_FL_INDEXED_NAME 3    /* 01NTxxxx  name ref + value literal  */
#define QH_FL_INDEXED_NAME_PB 4 /* 0000Nxxx  post-base name ref + value */
#define QH_FL_LITERAL 5         /* 001NHxxx  name literal + value      */
#define QH_ES_INSERT_INDEXED 6  /* 1Txxxxxx  insert with name ref      */
#define QH_ES_INSERT 7          /* 01Hxxxxx  insert with literal name  */
#define QH_ES_SET_DTABLE_CAP 8  /* 001xxxxx                            */
#define QH_ES_DUPLICATE 9       /* 000xxxxx                            */

#define QH_FL_DYNAMIC 0x1u /* index refers to the dynamic table (T = 0) */
#define QH_FL_NEVER 0x2u   /* N bit: never index                        */

/* One field line or encoder instruction (24 B).  name / value are indices
 * into the span array of the same call, or -1. */
typedef struct qh_field_line {
  uint64_t index; /* table index / capacity as encoded; 0 for literals */
  uint8_t opcode; /* QH_FL_* or QH_ES_*                                */
  uint8_t flags;  /* QH_FL_DYNAMIC | QH_FL_NEVER                        */
  uint16_t reserved;
  int32_t name;
  int32_t value;
  uint32_t reserved2;
} qh_field_line;

/* Encoded field section prefix (RFC 9204 4.5.1, qpack.c:3369-3437). */
typedef struct qh_section_prefix {
  uint64_t ricnt;      /* Encoded Required Insert Count (not reconstructed) */
  uint64_t delta_base;
  uint32_t sign;
  uint32_t reserved;
} qh_section_prefix;

/* Scans one complete field section (fin = 1).  Returns 0, or the error
 * nghttp3_qpack_decoder_read_request would return for it:
 * QH_ERR_QPACK_DECOMPRESSION_FAILED (integer overflow, a representation cut
 * by the end of the section, :3780-3784, or an index no table state can
 * make valid: a static index >= 99, :3992 -> :2796-2797; with Required
 * Insert Count 0 a negative Delta Base, :3414-3418, or any dynamic
 * reference, :3985-3987, :4009-4011), QH_ERR_QPACK_HEADER_TOO_LARGE
 * (name > 256 / value > 65536 bytes, Huffman ones by their len*8/5
 * estimate, :3575-3588, :3661-3674), or QH_ERR_NOMEM when lines_cap /
 * spans_cap is too small.  On an error *nlines is 0 and *nspans counts the
 * strings read before it (the reference decodes those first, so a Huffman
 * failure among them takes precedence: -401).  Span offsets are src_off +
 * position in src.  Indices are not resolved: a section with a non-zero
 * Required Insert Count frames fine whatever the dynamic table holds. */
QH_EXPORT int qh_qpack_scan_field_section(
    const uint8_t *src, size_t srclen, uint64_t src_off,
    qh_section_prefix *prefix, qh_field_line *lines, size_t lines_cap,
    size_t *nlines, qh_span_in *spans, size_t spans_cap, size_t *nspans);

/* Batch of field sections: block i is src[blocks[i].off, +len).  Lines and
 * spans of block i are [line_start[i], line_start[i+1]) and likewise for
 * spans (both arrays hold nblocks + 1 entries); status[i] is block i's
 * framing verdict (a failed block contributes no lines, and the spans it
 * read before the error).  Returns 0, or QH_ERR_NOMEM when the caps are
 * exceeded. */
QH_EXPORT int qh_qpack_scan_blocks(const uint8_t *src,
                                   const qh_span_in *blocks, size_t nblocks,
                                   qh_field_line *lines, size_t lines_cap,
                                   qh_span_in *spans, size_t spans_cap,
                                   uint32_t *line_start, uint32_t *span_start,
                                   int32_t *status);

/* The same batch scan on the GPU (blocks, lines, spans, line_start,
 * span_start, status and huff in HBM; where must be QH_WHERE_DEVICE): same
 * parser source, same outputs and verdicts as qh_qpack_scan_blocks.  If
 * huff is not NULL it also receives the Huffman-coded spans alone, in
 * order, ready for qh_decode_batch.  totals (host, may be NULL) receives
 * {lines, spans, Huffman spans}.  Synchronises once (to check the totals
 * against the caps); returns 0, QH_ERR_NOMEM or QH_ERR_FATAL. */
QH_EXPORT int qh_scan_blocks_batch(qh_ctx *ctx, const uint8_t *src,
                                   const qh_span_in *blocks, size_t nblocks,
                                   qh_field_line *lines, size_t lines_cap,
                                   qh_span_in *spans, size_t spans_cap,
                                   uint32_t *line_start, uint32_t *span_start,
                                   int32_t *status, qh_span_in *huff,
                                   size_t huff_cap, uint64_t *totals,
                                   int where);

/* ---- Whole field sections in one call (decoder side of config 4) -------
 * Replaces the request-stream decode loop of nghttp3_qpack_decoder_read_request
 * (lib/nghttp3_qpack.c:3347-3805) for a batch of complete, independent field
 * sections (fin = 1 each): framing (the parser above), every Huffman string
 * decoded by the batch kernels (qpack_read_huffman_string, :2737-2763), a
 * Huffman failure turned into the block's DECOMPRESSION_FAILED (:3604-3609,
 * :3693-3698), then per string the field name / value check of
 * nghttp3_check_header_name / _value (http.c:691-709, :798-838) and, for
 * names, the token of qpack_lookup_token (qpack.c:342; the reference
 * computes it on emit, :4130).
 *
 * Outputs are caller-allocated (HBM for QH_WHERE_DEVICE, host memory for
 * QH_WHERE_HOST, where the call stages through the device and blocks):
 *   lines / spans / line_start / span_start / status -- as qh_qpack_scan_blocks
 *     (lines_cap, spans_cap >= total block bytes + 1 always suffice);
 *   strs[k]    -- string k: a Huffman string decoded into dst (off, len in
 *                 dst, status 0 or QH_ERR_QPACK_FATAL); a raw string is not
 *                 copied (off, len in src, status 0);
 *   verdict[k] -- 1 valid / 0 not (0 for a failed Huffman string); optional;
 *   token[k]   -- nghttp3_qpack_token of a name, -1 otherwise; optional;
 *   dst        -- decoded Huffman strings, qh_decode_batch's slot layout in
 *                 Huffman-string order; dst_cap >= the `dst_need` total.
 * status[b] is 0 or the reference's error for the block: its first framing
 * error, unless a Huffman string before it fails (-401).  A block whose
 * framing failed has no lines (its line_start range is empty) and keeps the
 * spans read before the error; a block that framed cleanly but whose
 * Huffman string failed (-401) keeps all its lines and spans -- the framing
 * is valid, the string's strs[k].status says which one failed -- where the
 * reference emits no field of it (the callers drop such a block's lines).
 * On QH_ERR_NOMEM the framing may have written lines and spans below the
 * caps; nothing else is written.
 * Totals (nlines, nspans, nhuff, dst_need) are filled in on return, also on
 * QH_ERR_NOMEM (caps or dst_cap too small: nothing was decoded; resize and
 * call again).  opts: QH_SECTIONS_DTABLE0 decodes as a decoder whose
 * dynamic table capacity is 0 (qpack_decode -s 0): any Required Insert
 * Count but 0 fails the block (reconstruct_ricnt, :3915-3950).
 *
 * QH_SECTIONS_PACKED (both `where` values) changes dst's layout and nothing
 * else: the decoded Huffman strings lie back to back in dst, in
 * Huffman-string order, strs[k].off of a successful Huffman string being
 * the sum of the decoded lengths of the successful Huffman strings before
 * it; a failed Huffman string takes no bytes (status QH_ERR_QPACK_FATAL,
 * len 0); raw strings still point into src.  lines, spans, line_start,
 * span_start, status, verdict, token, prefixes, nlines, nspans and nhuff
 * are byte for byte those of the call without the bit.
 * dst_cap >= (total block bytes) * 8 / 5 always suffices (every Huffman
 * string lies inside its block and decodes to at most len * 8 / 5 bytes).
 * On success dst_need is the exact number of packed bytes written.  If the
 * packed bytes would pass dst_cap the call returns QH_ERR_NOMEM with
 * dst_need set to the exact need and nothing written at or past dst_cap;
 * in that case (QH_SECTIONS_PACKED only) the other outputs are unspecified.
 * (When lines_cap or spans_cap is too small, QH_ERR_NOMEM comes from the
 * count as without the bit, nothing else written; dst_need then holds an
 * upper bound of the packed bytes, the slot layout's total.)
 * With QH_WHERE_HOST, QH_SECTIONS_PACKED and the caps that always suffice
 * (lines_cap, spans_cap >= total block bytes + 1, dst_cap >= total block
 * bytes * 8 / 5, lines / spans / strs given) the call is pipelined over
 * slices of consecutive blocks (QH_OPT_SECTIONS_SLICE_BLOCKS): a slice's
 * results go back to host memory while the next slices come in and are
 * decoded.  Any other host call counts everything first and keeps the
 * contract above (QH_ERR_NOMEM with the full totals, nothing else written).
 * Any other bit of opts gives QH_ERR_INVALID_ARGUMENT. */
#define QH_SECTIONS_DTABLE0 0x1u
#define QH_SECTIONS_PACKED 0x2u

typedef struct qh_sections {
  qh_field_line *lines;
  size_t lines_cap;
  qh_span_in *spans;
  size_t spans_cap;
  qh_span_out *strs;
  int8_t *verdict;
  int32_t *token;
  uint32_t *line_start; /* nblocks + 1 */
  uint32_t *span_start; /* nblocks + 1 */
  int32_t *status;      /* nblocks     */
  qh_section_prefix *prefixes; /* nblocks, optional: each block's prefix as
                                  encoded (zero for a block whose prefix
                                  does not parse) */
  uint8_t *dst;
  uint64_t dst_cap;
  /* filled in by the call */
  uint64_t nlines, nspans, nhuff, dst_need;
} qh_sections;

QH_EXPORT int qh_decode_sections_batch(qh_ctx *ctx, const uint8_t *src,
                                       const qh_span_in *blocks,
                                       size_t nblocks, uint32_t opts,
                                       qh_sections *out, int where);

/* Scans encoder-stream bytes.  Returns the number of bytes of complete
 * instructions (a trailing partial instruction is left for the next call,
 * like the streaming decoder), QH_ERR_QPACK_ENCODER_STREAM_ERROR (also for
 * a static name reference >= 99, qpack.c:2916 -> :3965-3966),
 * QH_ERR_QPACK_HEADER_TOO_LARGE or QH_ERR_NOMEM. */
QH_EXPORT nghttp3_ssize qh_qpack_scan_encoder_stream(
    const uint8_t *src, size_t srclen, uint64_t src_off, qh_field_line *insts,
    size_t insts_cap, size_t *ninsts, qh_span_in *spans, size_t spans_cap,
    size_t *nspans);

/* Prefixed integers, qpack.c:2643-2682 (nghttp3_qpack_put_varint_len /
 * nghttp3_qpack_put_varint). */
QH_EXPORT size_t qh_qpack_put_varint_len(uint64_t n, size_t prefix);
QH_EXPORT uint8_t *qh_qpack_put_varint(uint8_t *buf, uint64_t n,
                                       size_t prefix);

/* Representation writers; each returns the bytes written at dst.  fb is the
 * first byte's fixed bits and prefix the index / name-length prefix, as the
 * reference's callers pass them (qpack.c:1898-2069): indexed static 0xc0/6,
 * dynamic 0x80/6, post-base 0x10/4; name ref static 0x50/4 (| 0x20 never),
 * dynamic 0x40/4, post-base 0x00/3 (| 0x08); literal 0x20/3 (| 0x10);
 * inserts 0xc0/6, 0x80/6 (name ref) and 0x40/5 (literal name).  Strings
 * are Huffman-coded iff that is strictly shorter (:1862, :1954, :1962).
 * dst must hold qh_qpack_literal_bound(namelen, valuelen) bytes. */
QH_EXPORT size_t qh_qpack_write_indexed(uint8_t *dst, uint8_t fb,
                                        uint64_t idx, size_t prefix);
/* qpack_encoder_write_indexed_name, qpack.c:1851-1896 */
QH_EXPORT size_t qh_qpack_write_indexed_name(uint8_t *dst, uint8_t fb,
                                             uint64_t nameidx, size_t prefix,
                                             const uint8_t *value,
                                             size_t valuelen);
/* qpack_encoder_write_literal, qpack.c:1944-2006 */
QH_EXPORT size_t qh_qpack_write_literal(uint8_t *dst, uint8_t fb,
                                        size_t prefix, const uint8_t *name,
                                        size_t namelen, const uint8_t *value,
                                        size_t valuelen);
QH_EXPORT size_t qh_qpack_literal_bound(size_t namelen, size_t valuelen);

/* Batch writer of whole field sections (the encoder side of config 4):
 * section b is lines [line_start[b], line_start[b + 1]) (QH_FL_* opcodes;
 * name / value index `strs`, spans of `plain`) after its prefix (all zero
 * if prefixes is NULL).  sections[b] receives the section's (off, len) in
 * dst.  Returns 0, QH_ERR_NOMEM (dst_cap too small) or
 * QH_ERR_INVALID_ARGUMENT (unknown opcode / missing string). */
QH_EXPORT int qh_qpack_write_sections(const uint8_t *plain,
                                      const qh_span_in *strs,
                                      const qh_field_line *lines,
                                      const uint32_t *line_start,
                                      size_t nsections,
                                      const qh_section_prefix *prefixes,
                                      uint8_t *dst, size_t dst_cap,
                                      qh_span_in *sections);

/* ---- The encoder side of whole field sections (SURVEY.md section 8(a)
 * rows a9 / a10, 8(f) row 2) ----------------------------------------------
 * The static table (RFC 9204 Appendix A; the reference's stable[],
 * qpack.c:189-291): entry idx's name and value (static storage). */
QH_EXPORT int qh_qpack_static_entry(size_t idx, const uint8_t **name,
                                    size_t *namelen, const uint8_t **value,
                                    size_t *valuelen);

/* The representation nghttp3_qpack_encoder_encode_nv (qpack.c:1455-1628)
 * chooses for each of nfields fields when the dynamic table is not used
 * (capacity 0; qpack_encode -s 0): field i is strs[2i] (name) and
 * strs[2i + 1] (value), spans of `plain`; never[i] (optional) is its
 * NGHTTP3_NV_FLAG_NEVER_INDEX.  lines[i] becomes an Indexed Field Line
 * (static entry with that name and value), a Literal With (static) Name
 * Reference, or a Literal With Literal Name, with name / value = 2i / 2i + 1
 * where used and QH_FL_NEVER from never[i] (the static lookup also skips the
 * value match for authorization and cookie values under 20 bytes,
 * :1307-1321, :1643-1645).  Host C. */
QH_EXPORT int qh_qpack_plan_fields(const uint8_t *plain, const qh_span_in *strs,
                                   size_t nfields, const uint8_t *never,
                                   qh_field_line *lines);

/* Batch writer of whole field sections on the GPU: the encoder batch
 * adapter of the Huffman call sites (qpack.c:1851-2006).  Section b is
 * lines [line_start[b], line_start[b + 1]) after its prefix (prefixes[b], or
 * all zero when prefixes is NULL: no dynamic-table references); a line's
 * name / value index strs, spans of plain.  Steps: hlen of every string
 * (the count kernels), Huffman iff hlen < len (:1862, :1954, :1962), the
 * picked strings encoded densely (the encode kernels), then the sections
 * written (first bytes and prefixes as qh_qpack_write_sections; byte for
 * byte its output).  sections[b] receives (off, len) in dst, sections back
 * to back from 0; *dst_need the total.  All pointers in HBM
 * (QH_WHERE_DEVICE; one sync, for the caps check) or in host memory
 * (QH_WHERE_HOST: staged, blocking).  Returns 0, QH_ERR_NOMEM (dst_cap <
 * *dst_need; nothing written), QH_ERR_INVALID_ARGUMENT (unknown opcode or
 * missing string) or QH_ERR_FATAL. */
QH_EXPORT int qh_encode_sections_batch(qh_ctx *ctx, const uint8_t *plain,
                                       const qh_span_in *strs, size_t nstrs,
                                       const qh_field_line *lines,
                                       const uint32_t *line_start,
                                       size_t nsections,
                                       const qh_section_prefix *prefixes,
                                       uint8_t *dst, uint64_t dst_cap,
                                       qh_span_in *sections,
                                       uint64_t *dst_need, int where);

/* ---- Field name / value validation -------
 * Scalar drop-ins for the public functions (nghttp3.h:3443, :3452;
 * lib/nghttp3_http.c:691-709, :798-838), nghttp3_amd/csrc/qh_http.c. */
QH_EXPORT int nghttp3_check_header_name(const uint8_t *name, size_t len);
QH_EXPORT int nghttp3_check_header_value(const uint8_t *value, size_t len);

/* Batch form on the GPU: verdict[i] = nghttp3_check_header_name of string i
 * if in[i].flags has QH_SPAN_NAME, else nghttp3_check_header_value (1 valid,
 * 0 not), e.g. over the decode destination right after qh_decode_batch.
 * Device strings are read in aligned 16-byte chunks that each hold a byte
 * of the string (so no load leaves the string's pages; no padding is
 * needed).  Host batches are staged. */
QH_EXPORT int qh_check_fields_batch(qh_ctx *ctx, const uint8_t *src,
                                    const qh_span_in *in, size_t n,
                                    int8_t *verdict, int where);

/* ---- Header-name tokens ------------------
 * qh_qpack_lookup_token replaces the static qpack_lookup_token
 * (lib/nghttp3_qpack.c:342, generated by genlibtokenlookup.py): the
 * nghttp3_qpack_token of a field name (nghttp3.h:840-1131), or -1.  The
 * batch form looks up every string of a batch on the GPU (names decoded by
 * qh_decode_batch stay in HBM). */
QH_EXPORT int32_t qh_qpack_lookup_token(const uint8_t *name, size_t namelen);
QH_EXPORT int qh_lookup_tokens_batch(qh_ctx *ctx, const uint8_t *src,
                                     const qh_span_in *in, size_t n,
                                     int32_t *token, int where);

/* ---- The decoder's dynamic table and field emission ---------------------
 * What nghttp3_qpack_decoder_read_request hands its caller after the steps
 * above: a list of (name, value, token, flags) per field section, every
 * index resolved against the static table and a dynamic table state.
 *
 * The dynamic table (host C, csrc/qh_emit.c) replaces the decoder side of
 * nghttp3_qpack_decoder_read_encoder's effects: set_max_dtable_capacity
 * (lib/nghttp3_qpack.c:3159-3185), rel2abs (:3952-3969), the inserts
 * (:3187-3306) and the eviction of context_dtable_add (:2071-2127).  It is
 * kept as an append-only log: entry a (absolute index) is record
 * entries[ent_base + a], its name and value bytes [name_off, +name_len) and
 * [value_off, +value_len) of the byte log.  Entries and bytes are only ever
 * appended, so a view (one table state) taken earlier stays valid after
 * later qh_dtable_apply calls, and `entries` / `bytes` prefixes uploaded
 * earlier stay valid on the device (the arrays themselves may move when
 * they grow: read the pointers again after an apply). */
typedef struct qh_dyn_entry { /* 32 B */
  uint64_t name_off, value_off;
  uint32_t name_len, value_len;
  int32_t token; /* qh_qpack_lookup_token(name) at insert */
  uint32_t reserved;
} qh_dyn_entry;

typedef struct qh_dtable_view { /* one table state, 40 B */
  int64_t ent_base;      /* entry a is entries[ent_base + a]              */
  uint64_t live_lo;      /* lowest absolute index not evicted             */
  uint64_t insert_count; /* next_absidx (qpack.c:2787-2798: an index is
                            valid iff live_lo <= a < insert_count)        */
  uint64_t max_entries;  /* hard_max_dtable_capacity / 32 (:3915-3950)    */
  uint64_t reserved;
} qh_dtable_view;

typedef struct qh_dtable qh_dtable;

/* A table whose hard maximum capacity, and initial capacity, is hard_max
 * (nghttp3_qpack_decoder_init + the CLI's set_max_dtable_capacity). */
QH_EXPORT int qh_dtable_new(qh_dtable **pdt, uint64_t hard_max);
QH_EXPORT void qh_dtable_del(qh_dtable *dt);
/* Applies encoder-stream instructions as qh_qpack_scan_encoder_stream wrote
 * them (insts, spans; string k is src[spans[k].off, +len), or, if
 * spans[k].flags has QH_SPAN_HUFFMAN, the decoded bytes dec[strs[k].off,
 * +strs[k].len) -- decoded by the caller with the scalar drop-in or
 * qh_decode_batch; dec / strs may be NULL when no string is Huffman-coded).
 * Returns 0, or QH_ERR_QPACK_ENCODER_STREAM_ERROR at the first failing
 * instruction with the earlier ones applied: a capacity above the hard
 * maximum (:3163-3165), an entry larger than the capacity (:2085-2087 via
 * :3187-3306), a relative index that is not live or a static index >= 99
 * (:3952-3969).  QH_ERR_NOMEM when the log cannot grow. */
QH_EXPORT int qh_dtable_apply(qh_dtable *dt, const qh_field_line *insts,
                              size_t ninsts, const uint8_t *src,
                              const qh_span_in *spans, const uint8_t *dec,
                              const qh_span_out *strs);
/* The current state, and the logs (*n: records / bytes so far). */
QH_EXPORT int qh_dtable_get_view(const qh_dtable *dt, qh_dtable_view *view);
QH_EXPORT const qh_dyn_entry *qh_dtable_entries(const qh_dtable *dt, size_t *n);
QH_EXPORT const uint8_t *qh_dtable_bytes(const qh_dtable *dt, size_t *n);

/* ---- Many dynamic tables in one log: encoder streams in batches ---------
 * nghttp3_qpack_decoder_read_encoder (qpack.c:2815-3306) for a batch of
 * connections.  A table is two records in caller-owned arrays, views[t] (as
 * emission and the planners take it) and acct[t], over one shared log:
 * entries[0, *nentries) and bytes[0, *nbytes), caller-owned, append-only.
 * There is no library object.
 *
 * One call applies stream p = src[streams[p].off, +len) to table tsel[p]
 * (tsel NULL: table p, nsel = ntables).  Per stream the instructions are
 * applied in order; a trailing partial instruction is not consumed
 * (consumed[p] = the bytes of complete, applied instructions: hand the rest
 * in again with what follows).  The first failing instruction sets
 * status[p], the ones before it stay applied and consumed[p] ends before it:
 * QH_ERR_QPACK_ENCODER_STREAM_ERROR for a capacity above hard_max, an entry
 * larger than the capacity, a relative index that is not live, a static
 * index >= 99, a varint overflow, or a Huffman string that does not decode
 * (EOS, padding: qpack.c:2737-2763); QH_ERR_QPACK_HEADER_TOO_LARGE exactly
 * as qh_qpack_scan_encoder_stream reports it.
 *
 * Layout rule (the host function and the kernels follow it, so their logs
 * are byte for byte equal).  Allocation follows the order of the call's
 * table list.  A table moves iff at least one insert or duplicate of its
 * stream is applied.  A moving table's records live on entry, [live_lo,
 * insert_count) on entry, L of them, are copied verbatim (offsets
 * unchanged) to the entry cursor, one record per applied insert follows in
 * stream order, and ent_base becomes region_start - live_lo (on entry): entry
 * a is still entries[ent_base + a] for every a live on entry and every new
 * one.  Its bytes go to the byte cursor back to back, per applied insert the
 * name bytes (a literal or static name; a dynamic name reference or a
 * duplicate shares the old offsets) and then the value bytes (unless a
 * duplicate).  A table that does not move (an empty stream, set-capacity
 * only, a failure before the first insert) keeps ent_base; live_lo, cap and
 * size still change as the instructions say.  Records and bytes written
 * earlier are never modified, so a view copied before the call stays valid
 * after it.
 * Growth: a call appends, per moving table, 32 (L + inserts) bytes of records
 * and the new strings' bytes; the records of the regions left behind stay.
 * A table of capacity C holds at most C / 32 live records, so relocation
 * costs at most C bytes per touched table per call.  The regions left behind
 * are given back by compacting the log (qh_qpack_dtables_compact /
 * qh_dtables_compact_batch below: the live records copied to a fresh log,
 * views rebased); when to do so is the caller's decision.
 *
 * Returns 0; QH_ERR_INVALID_ARGUMENT (a table index >= ntables, a table
 * listed twice in tsel: nothing is written); QH_ERR_NOMEM when entries_cap
 * or bytes_cap is too small: *nentries and *nbytes are then the exact sizes
 * the log would have, views, acct and the log are untouched (status and
 * consumed may have been written), and the caller grows the arrays and calls
 * again with its old counts.  A view whose live range leaves the log, or a
 * referenced record whose strings leave [0, *nbytes), fails that table with
 * QH_ERR_QPACK_ENCODER_STREAM_ERROR and nothing is read outside the log. */
typedef struct qh_dtable_acct { /* 32 B: what an apply needs and a view does not */
  uint64_t hard_max; /* the hard maximum capacity                           */
  uint64_t cap;      /* the current capacity                                */
  uint64_t size;     /* sum of name_len + value_len + 32 over live entries  */
  uint64_t reserved;
} qh_dtable_acct;

/* A fresh table (nghttp3_qpack_decoder_init + set_max_dtable_capacity). */
QH_EXPORT void qh_dtable_state_init(uint64_t hard_max, qh_dtable_view *view,
                                    qh_dtable_acct *acct);

QH_EXPORT int qh_qpack_dtables_apply(
    const uint8_t *src, const qh_span_in *streams, const uint32_t *tsel, size_t nsel,
    size_t ntables, qh_dtable_view *views, qh_dtable_acct *acct, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes,
    uint64_t bytes_cap, int32_t *status, uint32_t *consumed);

/* The same over arrays in HBM (where must be QH_WHERE_DEVICE; nentries and
 * nbytes are host scalars).  Asynchronous on the context stream after one
 * host wait, which reads the parser's totals and the size pass's totals
 * (against the caps): the work is queued over scratch laid out from what the
 * context's previous call parsed, scaled to this call's stream count plus an
 * eighth, and a call that parses more than that (and the first one) waits
 * twice.  A call much smaller per stream than the one before it pays for the
 * unused layout once (a memset and empty strings for the decoder).  No
 * fence is needed inside the apply kernel: one lane per table walks, and the
 * only records of this call it reads back are the ones it stored itself; the
 * bytes a call appends are not read by that call.  Sources are read in place:
 * no padding is required around src.  Scratch comes from the context. */
QH_EXPORT int qh_dtables_apply_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *streams, const uint32_t *tsel, size_t nsel,
    size_t ntables, qh_dtable_view *views, qh_dtable_acct *acct, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes,
    uint64_t bytes_cap, int32_t *status, uint32_t *consumed, int where);

/* Compaction of the shared log: the live records of the listed views copied
 * to a fresh log (entries_out, bytes_out: caller-owned, not overlapping the
 * source arrays), the views rewritten in place to point into it.  `views` is
 * any list of views into the source log: normally the set's views array; a
 * caller that still needs an older snapshot of a table (a view copied for a
 * blocked section) appends it.  Every listed view gets its own region, so a
 * snapshot costs a second copy of the records it shares with the current
 * view (overlapping views are not merged).  acct is not an argument: nothing
 * in it changes.  No policy is built in: the caller compares *nentries and
 * *nbytes of its log with what its tables can hold and decides when to call.
 *
 * Layout rule of the compacted log (the host function and the kernels follow
 * it, so their outputs are byte for byte equal).  Views are taken in list
 * order.  View t has L_t = insert_count - live_lo live records; they go to
 * entries_out[E_t, E_t + L_t) in absolute-index order, E_t the sum of L_u
 * over u < t, and its ent_base becomes E_t - live_lo (an empty view's too);
 * live_lo, insert_count, max_entries and reserved are unchanged.  Bytes are
 * unshared: output record r (counted over the whole list, views in order,
 * records in order) owns bytes_out[B_r, B_r + name_len + value_len), B_r the
 * sum of name_len + value_len over the records before it; name_off = B_r,
 * value_off = B_r + name_len (empty strings too); name_len, value_len, token
 * and reserved are copied.  A duplicate or a dynamic name reference, which
 * shared bytes with an older entry in the source log, gets its own copy.
 * So *nbytes_out is the sum over the views of size_t - 32 L_t (size_t: the
 * table's accounted size), and a compacted log of current views is never
 * larger than the sum of the tables' capacities; no dedupe pass is needed;
 * and the result does not depend on which entries happened to share bytes.
 * The source arrays are only read: a view copied before the call stays valid
 * against the old arrays, which the caller frees when it no longer needs
 * them.  A hashed index (qh_dyn_index_batch below) names records by their
 * place in the log, so it does not survive this call: build it again over
 * the rewritten views.  The same holds for a table that an apply relocated
 * (its ent_base changed); until then the planners fall back to the scan for
 * that view by themselves, the record's ent_base no longer being the view's.
 *
 * Returns 0 with the views rewritten and *nentries_out / *nbytes_out the
 * compacted log's lengths (nviews == 0 or every view empty: 0 and 0; null
 * outputs are allowed then).  QH_ERR_NOMEM when entries_out_cap or
 * bytes_out_cap is too small: *nentries_out and *nbytes_out are the exact
 * needs, views and outputs are untouched (caps of 0 with null outputs is the
 * sizing call).  QH_ERR_INVALID_ARGUMENT with nothing written to views,
 * outputs or the two counts when a view fails against nentries (its live
 * range leaves the log) or a live record's strings leave [0, nbytes) (or its
 * two lengths sum to 2^32 or more, which no apply writes): status[t] is then
 * QH_ERR_INVALID_ARGUMENT for each offending view and 0 for the others
 * (status may be written on the error paths).  QH_ERR_INVALID_ARGUMENT also
 * when the output arrays overlap the source arrays, a pointer is null where
 * its count is not 0, or nviews is above 2^27 - 1 (the apply's grid limit).
 * Nothing is read outside [0, nentries) or [0, nbytes), nothing is written at
 * or past *nentries_out or *nbytes_out. */
QH_EXPORT int qh_qpack_dtables_compact(
    size_t nviews, qh_dtable_view *views, const qh_dyn_entry *entries, uint64_t nentries,
    const uint8_t *bytes, uint64_t nbytes, qh_dyn_entry *entries_out, uint64_t *nentries_out,
    uint64_t entries_out_cap, uint8_t *bytes_out, uint64_t *nbytes_out, uint64_t bytes_out_cap,
    int32_t *status);

/* The same over arrays in HBM (where must be QH_WHERE_DEVICE; nentries_out and
 * nbytes_out are host scalars; at most 2^32 - 1 output records).  The work is
 * flat over output records, not a lane per table.  Asynchronous on the context
 * stream after one host wait, which reads the record total, the byte total
 * and the error flags before anything is written to the outputs or the views.
 * The per-record pass is sized from the context's previous call plus an
 * eighth; the first call, and one with more output records than that, waits
 * twice.  Scratch (16 bytes per view and per output record) comes from the
 * context. */
QH_EXPORT int qh_dtables_compact_batch(
    qh_ctx *ctx, size_t nviews, qh_dtable_view *views, const qh_dyn_entry *entries,
    uint64_t nentries, const uint8_t *bytes, uint64_t nbytes, qh_dyn_entry *entries_out,
    uint64_t *nentries_out, uint64_t entries_out_cap, uint8_t *bytes_out, uint64_t *nbytes_out,
    uint64_t bytes_out_cap, int32_t *status, int where);

/* Where a field's name / value bytes are. */
#define QH_IN_SRC 0    /* raw string in the block bytes (off into src)     */
#define QH_IN_DST 1    /* decoded Huffman string (off into sections dst)   */
#define QH_IN_STATIC 2 /* off = static index (qh_qpack_static_entry)       */
#define QH_IN_DYN 3    /* off into the dynamic table's byte log            */
#define QH_IN_OUT 4    /* materialised: off into qh_emit.out               */

typedef struct qh_field { /* 32 B, one per emitted field line */
  uint64_t name_off, value_off;
  uint32_t name_len, value_len;
  int32_t token; /* nv->token, qpack.c:4028, :4067, :4090, :4130 */
  uint8_t name_where, value_where; /* QH_IN_* */
  uint8_t flags; /* QH_FL_NEVER (NGHTTP3_NV_FLAG_NEVER_INDEX) */
  uint8_t reserved;
} qh_field;

#define QH_EMIT_BLOCKED 1 /* status: Required Insert Count > insert_count,
                             qpack.c:3428-3433 */
#define QH_EMIT_QIF 0x1u  /* opts: out is QIF text, name TAB value LF per
                             field and one more LF per emitted block
                             (examples/qpack_decode.cc:179-190) */

/* Field emission: replaces the prefix handling of read_request
 * (reconstruct_ricnt qpack.c:3915-3950, Base :3414-3422, the blocked
 * verdict :3428-3433), brel2abs / pbrel2abs (:3971-4017) and the emit_*
 * functions (:4020-4136) for the blocks of a finished
 * qh_decode_sections_batch result `s` (prefixes given; src and blocks as in
 * that call).  Block b is decoded against views[block_view[b]] (views[0]
 * when block_view is NULL; no dynamic table -- hard maximum 0, insert count
 * 0 -- when views is NULL), whose entries are dyn_entries[ent_base + a] and
 * whose bytes are in dyn_bytes.  sel lists the blocks to emit, each at most
 * once (NULL: all, nsel = nblocks); every output is indexed by position in
 * sel.  Per selected block, in the reference's order:
 *   1. the prefix: a Required Insert Count that does not reconstruct, or a
 *      negative Base, gives -401 whatever the framing status is (a block
 *      whose prefix did not parse has an all-zero prefix and passes);
 *   2. ricnt > insert_count: QH_EMIT_BLOCKED, no fields -- also when the
 *      block's lines hold a framing or Huffman error, which the reference
 *      has not read yet;
 *   3. a sections status of -401 stays;
 *   4. status 0: every line's index is resolved (static < 99; base-relative
 *      base >= idx + 1; absidx < ricnt; live); the first failure gives -401
 *      and no fields, else one qh_field per line: name and token from the
 *      entry (indexed and name-reference lines; a static entry's token is
 *      its name's) or from strs / token of the line's name, value from the
 *      entry (indexed lines) or strs of the line's value; a literal string
 *      is QH_IN_DST if its span has QH_SPAN_HUFFMAN, else QH_IN_SRC;
 *      QH_FL_NEVER is carried over, indexed lines get 0 (:4029);
 *   5. -109: the reference validates an index as it reads it, before the
 *      value's length (:3537-3542), so an invalid index before the oversize
 *      string, or in the cut line itself, makes the verdict -401.
 * status[p] is 0, QH_EMIT_BLOCKED or the error; ricnt[p] (optional) the
 * reconstructed Required Insert Count (0 when it does not reconstruct);
 * fields [field_start[p], field_start[p + 1]) are block p's (empty for a
 * failed or blocked block).  With out != NULL every field's name and value
 * bytes are copied back to back into out in block, line, name-then-value
 * order (with QH_EMIT_QIF as QIF text) and the records say QH_IN_OUT;
 * out_blocks[p] (optional) is block p's bytes in out.  nfields, out_need
 * (the bytes out needs under opts, whether or not out is given) and
 * nblocked are filled in; when fields_cap or out_cap (out != NULL) is too
 * small the call returns QH_ERR_NOMEM with those totals exact, status and
 * ricnt written, nothing written to fields or out, and field_start /
 * out_blocks unspecified.
 * QH_ERR_INVALID_ARGUMENT: unknown opts bits, s->prefixes == NULL,
 * block_view without views.
 * qh_qpack_emit_fields is host C over host pointers; qh_emit_fields_batch
 * is the same over pointers in HBM (where must be QH_WHERE_DEVICE; `s` and
 * `e` themselves are host structs of device pointers), asynchronous on the
 * context stream after one host wait for the totals. */
typedef struct qh_emit {
  qh_field *fields;
  size_t fields_cap;     /* >= s->nlines always suffices */
  uint32_t *field_start; /* nsel + 1 */
  int32_t *status;       /* nsel */
  uint64_t *ricnt;       /* nsel, optional */
  uint8_t *out;          /* optional */
  uint64_t out_cap;
  qh_span_in *out_blocks; /* nsel, optional */
  /* filled in by the call */
  uint64_t nfields, out_need, nblocked;
} qh_emit;

QH_EXPORT int qh_qpack_emit_fields(
    const uint8_t *src, const qh_span_in *blocks, size_t nblocks,
    const qh_sections *s, const qh_dtable_view *views,
    const uint32_t *block_view, const qh_dyn_entry *dyn_entries,
    const uint8_t *dyn_bytes, const uint32_t *sel, size_t nsel, uint32_t opts,
    qh_emit *e);
QH_EXPORT int qh_emit_fields_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *blocks, size_t nblocks,
    const qh_sections *s, const qh_dtable_view *views,
    const uint32_t *block_view, const qh_dyn_entry *dyn_entries,
    const uint8_t *dyn_bytes, const uint32_t *sel, size_t nsel, uint32_t opts,
    qh_emit *e, int where);

/* ---- Field representations on the GPU (SURVEY.md section 8(a) rows a9 /
 * a10) -------------------------------------------------------------------
 * qh_qpack_plan_fields on the GPU: the choice of
 * nghttp3_qpack_encoder_encode_nv at capacity 0 (qpack.c:1455-1628), its
 * indexing mode (:1307-1371) and nghttp3_qpack_lookup_stable (:1630-1660)
 * for every field of a batch, one lane per field; lines byte for byte those
 * of the host function (same source, csrc/qh_plan_core.h).
 * QH_WHERE_DEVICE: all pointers in HBM, asynchronous on the context stream,
 * no host wait.  QH_WHERE_HOST: staged, blocking.  Strings are read as
 * qh_check_fields_batch reads them (no padding is needed).  nfields may be
 * at most 2^30 (a line's name / value index is an int32). */
QH_EXPORT int qh_plan_fields_batch(qh_ctx *ctx, const uint8_t *plain,
                                   const qh_span_in *strs, size_t nfields,
                                   const uint8_t *never, qh_field_line *lines,
                                   int where);

/* Fields to field sections in one call: section b is fields
 * [field_start[b], field_start[b+1]) (nsections + 1 entries, nfields in all:
 * field_start[nsections] must be nfields), planned as above (the token is
 * computed from the name as the reference does, :1477; of a qh_field only
 * name_off, name_len, value_off, value_len -- offsets into plain -- and
 * flags & QH_FL_NEVER are read), then written as qh_encode_sections_batch
 * writes them (qpack.c:1817-2069; prefixes all zero: no dynamic-table
 * reference is ever chosen).  Takes qh_emit_fields_batch's `fields`,
 * `field_start` and `out` as they are.  A section whose range is empty is
 * its two prefix bytes.  Returns and the QH_ERR_NOMEM contract are those of
 * qh_encode_sections_batch (*dst_need exact, nothing written);
 * QH_WHERE_DEVICE keeps that call's single host wait and adds none. */
QH_EXPORT int qh_encode_fields_batch(qh_ctx *ctx, const uint8_t *plain,
                                     const qh_field *fields, size_t nfields,
                                     const uint32_t *field_start,
                                     size_t nsections, uint8_t *dst,
                                     uint64_t dst_cap, qh_span_in *sections,
                                     uint64_t *dst_need, int where);

/* ---- Field representations against a dynamic table state ----------------
 * The choice nghttp3_qpack_encoder_encode_nv (qpack.c:1455-1628) makes when
 * nothing can be inserted: every insert and the duplicate sit behind
 * qpack_encoder_can_index_nv / _duplicate (:1518-1521, :1544, :1570-1574,
 * :1608), which end in qpack_encoder_can_index (:1378-1413) and answer 0
 * while the table has no room and its oldest entry is pinned by an
 * unacknowledged section (:1408-1410).  The choice is then a function of
 * the field, the table state and (krcnt, allow_blocking): references to
 * entries already in the table, in this order (static lookup :1630-1660,
 * dynamic lookup :1662-1685 over encoder_qpack_map_find :799-835):
 *   1. a static entry with the name and value: Indexed (static);
 *   2. the newest referenceable entry with the name and value: Indexed
 *      (dynamic), QH_FL_DYNAMIC, index = base - a - 1 (:1824-1837);
 *   3. a static name: Literal With Name Reference (static);
 *   4. the newest referenceable entry with the name: Literal With Name
 *      Reference (dynamic), index = base - a - 1 (:1911-1930), N from the
 *      field's flag alone;
 *   5. Literal With Literal Name.
 * Entry a is referenceable iff live_lo <= a < insert_count in the section's
 * view and a + 1 <= ref_limit (:816, :819).  In NEVER mode (the flag,
 * authorization, a cookie under 20 bytes, :1307-1321) no value is matched
 * (:1643-1645, :822-824): steps 1 and 2 do not apply.  base is the view's
 * insert_count (:1163); no index is post-base.
 * Per section: max_cnt / min_cnt = the largest / smallest a + 1 over the
 * entries its lines reference (0 / UINT64_MAX when there is none), what
 * qpack_encoder_add_stream_ref records (:1193-1194), and the prefix of
 * write_field_section_prefix (:2424-2460): ricnt = max_cnt ? max_cnt %
 * (2 * max_entries) + 1 : 0, sign 0, delta_base = base - max_cnt (so a
 * section without a dynamic reference has delta_base = base, as the
 * reference writes it).
 *
 * A key per log entry lets the lookup read an entry's bytes only when the
 * key already agrees (a hash never decides: the name's bytes, when its
 * token is -1, and the value's are always compared).  The log is
 * append-only, so keys are: keys[first, first + n) are computed from
 * entries[first, first + n); a caller extends its array as the log grows. */
typedef struct qh_dyn_key { /* 16 B, one per log entry */
  uint32_t name_id;    /* the token, or 0x80000000 | hash of the name bytes
                          when the token is -1 */
  uint32_t name_len, value_len;
  uint32_t value_hash; /* 32-bit hash of the value bytes */
} qh_dyn_key;

/* The table states of a planning call: a host struct; its pointers are host
 * pointers for the host function and QH_WHERE_HOST, HBM for QH_WHERE_DEVICE.
 * Section b is planned against views[section_view[b]]; an index >= nviews,
 * or a view whose max_entries is 0, plans as no table.  An entry is never
 * matched when its record lies outside [0, nentries) or its strings outside
 * [0, nbytes). */
typedef struct qh_plan_dyn {
  const qh_dtable_view *views;
  size_t nviews;
  const uint32_t *section_view; /* nsections; NULL: views[0] */
  const uint64_t *ref_limit;    /* nsections; NULL: the view's insert_count
                                   (blocking allowed); else krcnt */
  const qh_dyn_entry *dyn_entries;
  size_t nentries;
  const qh_dyn_key *dyn_keys; /* nentries */
  const uint8_t *dyn_bytes;
  uint64_t nbytes;
} qh_plan_dyn;

/* keys[first, first + n) of the log (entries, nentries; bytes, nbytes); an
 * entry whose strings do not lie in the log gets zero hashes.  Host C, and
 * on the GPU one lane per entry (strings read as qh_check_fields_batch reads
 * them; QH_WHERE_DEVICE asynchronous, QH_WHERE_HOST staged and blocking). */
QH_EXPORT int qh_qpack_dyn_keys(const qh_dyn_entry *entries, size_t nentries,
                                const uint8_t *bytes, uint64_t nbytes,
                                size_t first, size_t n, qh_dyn_key *keys);
QH_EXPORT int qh_dyn_keys_batch(qh_ctx *ctx, const qh_dyn_entry *entries,
                                size_t nentries, const uint8_t *bytes,
                                uint64_t nbytes, size_t first, size_t n,
                                qh_dyn_key *keys, int where);

/* The lines, prefixes and reference counts of nsections sections: section b
 * is fields [field_start[b], field_start[b + 1]) of (strs, never) as
 * qh_qpack_plan_fields takes them.  prefixes (nsections) is required when
 * nsections > 0; max_cnt / min_cnt (nsections) are optional.  With dyn ==
 * NULL or nviews == 0 the lines are qh_qpack_plan_fields's and the prefixes
 * all zero.  Host C; qh_plan_fields_dyn_batch is the same on the GPU, lines
 * byte for byte (csrc/qh_plan_core.h is the source of both), with no host
 * wait for QH_WHERE_DEVICE.  QH_ERR_INVALID_ARGUMENT: dyn_keys NULL with
 * nentries > 0, section_view without views, nfields > 2^30. */
QH_EXPORT int qh_qpack_plan_fields_dyn(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, qh_field_line *lines, qh_section_prefix *prefixes,
    uint64_t *max_cnt, uint64_t *min_cnt);
QH_EXPORT int qh_plan_fields_dyn_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, qh_field_line *lines, qh_section_prefix *prefixes,
    uint64_t *max_cnt, uint64_t *min_cnt, int where);

/* qh_encode_fields_batch with the plan above: the fields planned against
 * dyn into context scratch, the prefixes formed on the device, then the
 * sections written as qh_encode_sections_batch writes them.  max_cnt /
 * min_cnt (nsections, optional) are what the caller keeps to pin its
 * entries until the sections are acknowledged.  Returns and the
 * QH_ERR_NOMEM contract are qh_encode_sections_batch's; QH_WHERE_DEVICE
 * keeps that call's single host wait and adds none. */
QH_EXPORT int qh_encode_fields_dyn_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_field *fields, size_t nfields,
    const uint32_t *field_start, size_t nsections, const qh_plan_dyn *dyn,
    uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint64_t *max_cnt, uint64_t *min_cnt, int where);

/* ---- A hashed index over the keys: lookups that do not scan ---------------
 * What encoder_qpack_map_find walks (qpack.c:799-835): a hash chain instead
 * of every live key.  An index covers one view: the entries [lo, hi) of its
 * live range, cut to the records inside the log as a scan range is; n = hi -
 * lo.  It is a record (caller-owned, one per view, parallel to views) and a
 * region of a caller-owned uint32_t slots[] array that starts at slot_off and
 * holds four blocks: nbuckets name heads, nbuckets exact heads, n name links,
 * n exact links.  A slot value is (a - lo) + 1; 0 means none.  nbuckets is the
 * smallest power of two >= max(16, 2 n), cut to the largest power of two <=
 * max_buckets when max_buckets != 0; a view of more than 2^28 entries gets
 * nbuckets 0 and no region (it is scanned).  Both bucket functions read only
 * an entry's qh_dyn_key: the name chain hashes (name_id, name_len), the exact
 * chain (name_id, name_len, value_len, value_hash); no string byte is read to
 * build an index.  A chain lists its bucket's entries newest first; the
 * content is that of: for a from lo up to hi - 1, link[a] = head[b], head[b]
 * = a, once per chain kind -- byte for byte, whoever builds it.
 *
 * A lookup over a section's range [s.lo, s.hi) uses the view's index iff
 * nbuckets != 0, the record's ent_base is the view's, rec.lo <= s.lo and the
 * region lies inside [0, nslots); else it is the scan.  Entries of
 * [max(s.lo, rec.hi), s.hi), inserted after the build, are scanned first (an
 * older index of a log that has only grown stays usable); then the exact
 * chain, then, where the line still needs it, the name chain.  A key or a
 * chain only ever rules entries out: every match is verified as the scan
 * verifies it.  A chain walk takes at most n steps and a slot value above n
 * ends it, so whatever slots holds, a lookup may miss a match but reads
 * nothing outside the arrays and ends.
 *
 * An index names records of the log by position: it must be rebuilt after
 * qh_dtables_compact_batch, and for a table that an apply relocated (its
 * ent_base changed; the lookup then falls back to the scan by itself). */
typedef struct qh_dyn_index_rec { /* 48 B, one per view */
  int64_t ent_base;  /* the view's, when the index was built */
  uint64_t lo, hi;   /* the entries covered */
  uint64_t slot_off; /* the region's first slot */
  uint32_t nbuckets; /* a power of two; 0: no index */
  uint32_t reserved[3];
} qh_dyn_index_rec;

typedef struct qh_plan_dyn_index {
  const qh_dyn_index_rec *recs; /* nviews, parallel to dyn->views */
  const uint32_t *slots;
  uint64_t nslots;
} qh_plan_dyn_index;

/* Builds the indexes of views vsel[0, nsel) (vsel NULL: every view, nsel
 * ignored) over keys[0, nentries): recs[v] is written per listed view, its
 * region allocated from *nslots on, in list order; *nslots becomes the slots
 * in use.  Returns 0; QH_ERR_INVALID_ARGUMENT for an index >= nviews or a
 * view listed twice (nothing is written); QH_ERR_NOMEM when slots_cap is
 * short, with *nslots the exact need (nothing else is written).  Host C;
 * qh_dyn_index_batch is the same on the GPU, recs and slots byte for byte:
 * QH_WHERE_DEVICE takes HBM pointers and a host nslots, and waits once, for
 * the total; QH_WHERE_HOST is staged and blocking. */
QH_EXPORT int qh_qpack_dyn_index(const qh_dtable_view *views, size_t nviews,
                                 const uint32_t *vsel, size_t nsel,
                                 const qh_dyn_key *keys, size_t nentries,
                                 uint32_t max_buckets, qh_dyn_index_rec *recs,
                                 uint32_t *slots, uint64_t *nslots,
                                 uint64_t slots_cap);
QH_EXPORT int qh_dyn_index_batch(qh_ctx *ctx, const qh_dtable_view *views,
                                 size_t nviews, const uint32_t *vsel,
                                 size_t nsel, const qh_dyn_key *keys,
                                 size_t nentries, uint32_t max_buckets,
                                 qh_dyn_index_rec *recs, uint32_t *slots,
                                 uint64_t *nslots, uint64_t slots_cap,
                                 int where);

/* qh_qpack_plan_fields_dyn, qh_plan_fields_dyn_batch and
 * qh_encode_fields_dyn_batch with the lookups through `index` (a host
 * struct; its pointers live where dyn's do): the same lines, prefixes,
 * counts and sections, byte for byte.  index == NULL: the calls above.  The
 * device forms add no host wait. */
QH_EXPORT int qh_qpack_plan_fields_dyn_indexed(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, const qh_plan_dyn_index *index,
    qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt);
QH_EXPORT int qh_plan_fields_dyn_indexed_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *never, const uint32_t *field_start, size_t nsections,
    const qh_plan_dyn *dyn, const qh_plan_dyn_index *index,
    qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, int where);
QH_EXPORT int qh_encode_fields_dyn_indexed_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_field *fields, size_t nfields,
    const uint32_t *field_start, size_t nsections, const qh_plan_dyn *dyn,
    const qh_plan_dyn_index *index, uint8_t *dst, uint64_t dst_cap,
    qh_span_in *sections, uint64_t *dst_need, uint64_t *max_cnt,
    uint64_t *min_cnt, int where);

/* ---- The encoder with dynamic-table inserts, for many connections --------
 * nghttp3_qpack_encoder_encode (qpack.c:1139-1204) for a batch of
 * connections, bit-exact: per connection its sections, and their fields, are
 * walked in order; per section process_dtable_update (:1240-1270, with
 * shrink_dtable :978-1009), base = insert_count (:1163), allow_blocking
 * (:1166-1170), then per field encode_nv in full (:1455-1628:
 * decide_indexing_mode :1307-1371 with both indexing strategies and
 * NGHTTP3_NV_FLAG_TRY_INDEX, lookup_stable :1630-1660, encoder_qpack_map_find
 * :799-835 with can_reference :791-795 and the post-base match that
 * suppresses an insert :1513-1514, check_draining :1446-1453, can_index
 * :1378-1413, the four dtable_*_add paths over context_dtable_add
 * :2071-2127, the writers' index arithmetic :1824-1837, :1911-1930,
 * :2019-2069), the section prefix with its sign (:2424-2460) and the
 * acknowledgement scalars moved as add_stream_ref would move them
 * (:1024-1074).  Connections are independent: the batch is parallel over
 * connections and sequential inside one.
 *
 * A connection is three records in caller-owned arrays over the shared log
 * of qh_qpack_dtables_apply: views[t], acct[t] (acct.cap is the encoder's
 * ctx.max_dtable_capacity) and enc[t].  There is no library object.
 * Acknowledgement bookkeeping is outside this call (per-stream reference
 * queues, ack_header, add_icnt, cancel_stream, the decoder-stream parser):
 * qh_enc_sec_flags_batch, qh_enc_refs_record_batch and
 * qh_enc_read_decoder_batch (below) do it over a reference log in HBM.  A
 * caller that keeps its own queues instead updates, between calls, krcnt,
 * pin_min, nblocked and nstreams from the max_cnt / min_cnt a call returns,
 * and per section it passes sec_flags.
 * Inside one call a connection's sections must belong to distinct streams
 * (otherwise split the call).  After a section with max_cnt > 0: pin_min =
 * min(pin_min, min_cnt), nstreams += !KNOWN, nblocked += (max_cnt > krcnt &&
 * !BLOCKED).  With QH_ENC_IMMEDIATE_ACK, after every section krcnt =
 * insert_count, pin_min = UINT64_MAX, nblocked = nstreams = 0
 * (ack_everything, :2385-2393). */
#define QH_ENC_IMMEDIATE_ACK 0x1u /* enc.flags: acknowledge every section at once */
#define QH_ENC_STRAT_NONE 0x2u    /* NGHTTP3_QPACK_INDEXING_STRAT_NONE (else EAGER) */
#define QH_ENC_CAP_PENDING 0x4u   /* ..._FLAG_PENDING_SET_DTABLE_CAP */

#define QH_ENC_SEC_STREAM_BLOCKED 0x1u /* sec_flags: its stream is blocked on entry */
#define QH_ENC_SEC_STREAM_KNOWN 0x2u   /* its stream has unacknowledged sections */

#define QH_NV_NEVER_INDEX 0x1u /* nvflags: NGHTTP3_NV_FLAG_NEVER_INDEX */
#define QH_NV_TRY_INDEX 0x2u   /* NGHTTP3_NV_FLAG_TRY_INDEX */

typedef struct qh_enc_state { /* 64 B */
  uint64_t krcnt;       /* known received count                                 */
  uint64_t pin_min;     /* smallest min_cnt over the unacknowledged sections,
                           UINT64_MAX for none (encoder_get_min_cnt, :969-976)  */
  uint64_t max_blocked; /* ctx.max_blocked_streams                              */
  uint64_t nblocked;    /* distinct blocked streams                             */
  uint64_t nstreams;    /* streams with unacknowledged sections (:1510: no
                           lookup at 2,000)                                     */
  uint64_t flags;       /* QH_ENC_*                                             */
  uint64_t min_update, last_update; /* :941-957 */
} qh_enc_state;

/* nghttp3_qpack_encoder_new at hard_max: capacity 0 (:847-861, :899-923). */
QH_EXPORT void qh_enc_state_init(uint64_t hard_max, uint64_t max_blocked, uint64_t flags,
                                 qh_dtable_view *view, qh_dtable_acct *acct, qh_enc_state *enc);
/* nghttp3_qpack_encoder_set_max_dtable_capacity (:941-957); the instruction
 * is written by the next call that encodes a section of the connection. */
QH_EXPORT void qh_enc_state_set_capacity(qh_enc_state *enc, qh_dtable_acct *acct, uint64_t cap);

/* Inputs: field i is strs[2i] (name) and strs[2i + 1] (value), spans of
 * plain, with nvflags[i] (QH_NV_*; NULL: 0); section b is fields
 * [field_start[b], field_start[b + 1]) with sec_flags[b] (NULL: 0);
 * connection c's sections are [conn_start[c], conn_start[c + 1]) (nconns + 1
 * entries, conn_start[0] = 0, conn_start[nconns] = nsections) and its table
 * is tsel[c] (NULL: table c, nconns = ntables).  A table named twice, or an
 * index >= ntables, gives QH_ERR_INVALID_ARGUMENT and no state is written.
 *
 * In/out: views, acct, enc; the log (entries, *nentries, entries_cap, bytes,
 * *nbytes, bytes_cap); keys, a qh_dyn_key per log entry, entries_cap of
 * them: keys[0, *nentries) are valid on entry and the call appends the keys
 * of what it appends.
 *
 * Out: lines[nfields] (field i's line: name / value = 2i / 2i + 1 where
 * used; post-base forms are QH_FL_INDEXED_PB / QH_FL_INDEXED_NAME_PB),
 * prefixes, max_cnt, min_cnt (per section); dst / sections: the field
 * sections back to back, section b at sections[b]; edst / estreams: one
 * encoder-stream span per listed connection (length 0 when it wrote
 * nothing); status[nconns].
 *
 * Log layout rule: qh_qpack_dtables_apply's, word for word.  Allocation
 * follows list order; a connection's table moves iff the call inserts or
 * duplicates into it; its records live on entry are copied verbatim to the
 * entry cursor (their keys too); one record per insert follows, in order;
 * per insert the name bytes (a literal or static name; a dynamic name
 * reference or a duplicate shares the old offsets), then the value bytes
 * (omitted for a duplicate); token is lookup_token of the name; nothing
 * written earlier is modified.  So, for a call with no pending capacity
 * reduction, the log, views and acct.size equal byte for byte what
 * qh_qpack_dtables_apply writes when given the emitted streams from the same
 * entry state.
 *
 * QH_ERR_NOMEM when any of entries_cap, bytes_cap, dst_cap, edst_cap is too
 * small: *nentries, *nbytes, *dst_need and *edst_need are the exact needs,
 * and views, acct, enc, keys and the log are untouched (the walk's results
 * live in scratch; caller-visible state is written by a final commit step).
 * On success they are the new lengths and the bytes written.
 * A view whose live range leaves the log, or a referenced record whose
 * strings leave [0, *nbytes), fails that connection only: status[c] =
 * QH_ERR_INVALID_ARGUMENT, its sections and its stream have length 0 (its
 * lines have opcode 0), its state is unchanged, nothing is read outside the
 * log.  A walk has at most fields + live entries eviction steps.
 * qh_qpack_encode_conns is host C over host pointers. */
QH_EXPORT int qh_qpack_encode_conns(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status);

/* The same over arrays in HBM (where must be QH_WHERE_DEVICE; nentries,
 * nbytes, dst_need and edst_need are host scalars): a connection per 16-lane
 * group walks (same source, csrc/qh_enc_core.h), the bytes are written by the
 * section writer of qh_encode_sections_batch, and a commit kernel writes the
 * log and the state once the four caps hold.  Three host waits: the walk's
 * record and byte totals, the section writer's sizes, the stream writer's
 * sizes.  Scratch (64 bytes per field, 24 per possible instruction) comes
 * from the context.  nfields at most 2^30, nconns at most 2^27 - 1. */
QH_EXPORT int qh_encode_conns_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *nvflags, const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    int where);

/* ---- The connection encoder's hashed index, kept up per insert -----------
 * What encoder_qpack_map_find walks (qpack.c:799-835) and ent->sum (:2106),
 * for the tables qh_qpack_encode_conns inserts into: a hash chain per bucket
 * in place of a scan of every live key, and can_reference, check_draining and
 * can_index from a running sum in O(1).  Opt-in per connection; a
 * qh_dyn_index_rec cannot serve here (it names records by log position, and
 * every inserting call moves the table).
 *
 * Entries are named by insert number a (the view's absolute index), never by
 * log position, so the index survives the relocation of an inserting call and
 * the rebasing of a compaction; it is never rebuilt.  One qh_enc_index_rec per
 * connection (caller-owned, beside views, acct and enc) owns a fixed region of
 * a caller-owned uint32_t slots[] array, sized once from acct.hard_max:
 *   ring      the smallest power of two >= max(16, hard_max / 32): an entry
 *             costs at least 32 bytes, so at most hard_max / 32 are live (under
 *             a pending capacity reduction too) and no two live entries share
 *             a mod ring.  ring == 0: the connection is scanned (hard_max / 32
 *             < min_entries, or more than 2^28).
 *   nbuckets  qh_qpack_dyn_index's rule over ring: the smallest power of two
 *             >= max(16, 2 ring), cut to the largest power of two <=
 *             max_buckets when that is not 0.
 * The region, from slot_off on, 2 nbuckets + 4 ring slots:
 *   [0, nbuckets)                 name heads, by qh_index_name_bucket
 *   [nbuckets, 2 nbuckets)        exact heads, by qh_index_exact_bucket
 *   then ring name links, ring exact links, and ring cumulative-space words
 *   of 64 bits (two slots, low half first), each at a mod ring.
 * A head or link value names an entry: 0 is none, else 0x80000000 | (a mod
 * 2^31), read back as the one number below the point it is read from (hi for
 * a head, the entry before for a link) with those 31 bits.  Entry a's
 * cumulative word is the space (name_len + value_len + 32) of the entries
 * inserted before it, from the oldest entry that was live when the index last
 * had no linked live entry (for a connection indexed since it was fresh: from
 * entry 0); only differences are used.  Linking entry a is, per chain kind,
 * link[a mod ring] = head[b]; head[b] = value(a), in insert order -- byte for
 * byte, host or device.  hi: every live entry below it is linked.
 *
 * Eviction writes nothing.  A value read on a chain is stale, and ends the
 * walk, when it names an entry below live_lo or one not older than the step
 * before (chains descend; a head's step before is hi).  A walk takes at most
 * ring steps; every slot read lies in the region, which is checked once
 * against nslots, and every log read in the live range.  So whatever slots
 * holds, a lookup may miss a match, but it reads nothing outside the arrays
 * and it ends.  A key or a chain only rules entries out: a match is verified
 * as the scan verifies it (key, lengths, the name's bytes when the token is
 * -1, the value's hash, the value's bytes).  A record that is unusable --
 * ring 0 or not a power of two, ring < hard_max / 32, nbuckets 0 or not a
 * power of two, a region outside [0, nslots), hi above the insert count --
 * makes its connection fall back to the scan, by itself.
 *
 * The lookup: entries of [hi, insert_count) (an un-indexed call ran in
 * between) and those inserted by this call are scanned newest first as ever;
 * below hi the exact chain is walked (not in never-index mode), then the name
 * chain when the line can still use a name (no exact match, no static name
 * reference).  The space from a candidate to the newest entry is size -
 * (cum[a] - cum[live_lo]).  The head sum of can_index is a difference of two
 * cumulative words.  (A record whose strings leave the byte log fails its
 * connection when a lookup reads it; the chains read fewer records than the
 * scan.) */
typedef struct qh_enc_index_rec { /* 32 B, one per connection */
  uint64_t slot_off; /* the region's first slot */
  uint64_t hi;       /* every live entry below it is linked */
  uint32_t ring;     /* a power of two; 0: the connection is scanned */
  uint32_t nbuckets; /* a power of two */
  uint64_t reserved;
} qh_enc_index_rec;

/* Sizes and allocates the regions of connections tsel[0, nsel) (NULL: every
 * connection, nsel ignored) from *nslots on, in list order, zeroes them, links
 * the entries live now (keys[0, nentries) are the log's) and writes recs[t]:
 * a set can adopt an index mid-life.  A connection with hard_max / 32 <
 * min_entries, or whose view leaves the log, gets ring 0 and no region.
 * *nslots becomes the slots in use.  QH_ERR_INVALID_ARGUMENT for an index >=
 * ntables or a connection listed twice, and QH_ERR_NOMEM when slots_cap is
 * short, *nslots then the exact need: nothing else is written.  Host C;
 * qh_enc_index_init_batch is the same over HBM pointers (where must be
 * QH_WHERE_DEVICE; nslots a host scalar), recs and slots byte for byte, and
 * waits once, for the total. */
QH_EXPORT int qh_qpack_enc_index_init(const qh_dtable_view *views, const qh_dtable_acct *acct,
                                      size_t ntables, const uint32_t *tsel, size_t nsel,
                                      const qh_dyn_key *keys, size_t nentries, uint64_t min_entries,
                                      uint32_t max_buckets, qh_enc_index_rec *recs, uint32_t *slots,
                                      uint64_t *nslots, uint64_t slots_cap);
QH_EXPORT int qh_enc_index_init_batch(qh_ctx *ctx, const qh_dtable_view *views,
                                      const qh_dtable_acct *acct, size_t ntables,
                                      const uint32_t *tsel, size_t nsel, const qh_dyn_key *keys,
                                      size_t nentries, uint64_t min_entries, uint32_t max_buckets,
                                      qh_enc_index_rec *recs, uint32_t *slots, uint64_t *nslots,
                                      uint64_t slots_cap, int where);

/* qh_qpack_encode_conns / qh_encode_conns_batch with the lookups through
 * recs[ntables] and slots[0, nslots): every output is the un-indexed call's
 * byte for byte (lines, prefixes, counts, sections, streams, status, views,
 * acct, enc, log, keys).  recs == NULL: the calls above.  The walk writes no
 * index; the commit, which runs only when the four caps hold, links every
 * entry of [max(hi, live_lo), insert_count) in insert order after relocating
 * and sets hi.  On QH_ERR_NOMEM, and for a failed connection, recs and slots
 * are untouched.  The device form adds no host wait. */
QH_EXPORT int qh_qpack_encode_conns_indexed(
    const uint8_t *plain, const qh_span_in *strs, size_t nfields, const uint8_t *nvflags,
    const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    qh_enc_index_rec *recs, uint32_t *slots, uint64_t nslots);
QH_EXPORT int qh_encode_conns_indexed_batch(
    qh_ctx *ctx, const uint8_t *plain, const qh_span_in *strs, size_t nfields,
    const uint8_t *nvflags, const uint32_t *field_start, size_t nsections, const uint8_t *sec_flags,
    const uint32_t *conn_start, size_t nconns, const uint32_t *tsel, size_t ntables,
    qh_dtable_view *views, qh_dtable_acct *acct, qh_enc_state *enc, qh_dyn_entry *entries,
    uint64_t *nentries, uint64_t entries_cap, uint8_t *bytes, uint64_t *nbytes, uint64_t bytes_cap,
    qh_dyn_key *keys, qh_field_line *lines, qh_section_prefix *prefixes, uint64_t *max_cnt,
    uint64_t *min_cnt, uint8_t *dst, uint64_t dst_cap, qh_span_in *sections, uint64_t *dst_need,
    uint8_t *edst, uint64_t edst_cap, qh_span_in *estreams, uint64_t *edst_need, int32_t *status,
    qh_enc_index_rec *recs, uint32_t *slots, uint64_t nslots, int where);

/* ---- Acknowledgements: the decoder stream read and written per batch -----
 * The encoder's side of nghttp3_qpack_encoder_read_decoder (qpack.c:2545-2641)
 * with ack_header (:2329-2372), add_icnt (:2374-2383), cancel_stream
 * (:2395-2412) and unblock (:2314-2327), the reference list of
 * qpack_encoder_add_stream_ref (:1024-1074) as the tail of encoder_encode
 * keeps it (:1183-1199), and the decoder's side:
 * nghttp3_qpack_decoder_write_section_ack (:3813-3839), write_decoder
 * (:3859-3887), decoder_cancel_stream (:3889-3913) and the acknowledgement at
 * the end of read_request (:3790-3795).
 *
 * State: connection t's unacknowledged sections are refs[rv[t].base, +
 * rv[t].n), oldest first, in one caller-owned log refs[0, *nrefs) of capacity
 * refs_cap; rv[] is a caller-owned array beside views, acct and enc.  dlen is
 * uninterrupted_decoderlen.  A fresh connection is all zeros.  There is no
 * library object.  Layout rules, the same on host and device:
 *   - a connection that gains references in a call moves: its references are
 *     copied in order to the cursor (*nrefs on entry, then past each moved
 *     connection in list order) and the new ones follow;
 *   - removal never moves a connection: its region is compacted in place,
 *     order kept, and n shrinks;
 *   - QH_ERR_NOMEM when refs_cap is too small: *nrefs is then the exact need
 *     and nothing is written;
 *   - qh_qpack_enc_refs_compact copies every listed connection's references
 *     back to back, in list order, into a fresh log (rv rebased), so the
 *     regions left behind are given back.  When to compact is the caller's
 *     decision, as for the dynamic-table log.
 * The derived scalars of qh_enc_state: pin_min is the smallest min_cnt left
 * (UINT64_MAX for none), nstreams the distinct stream ids left, nblocked the
 * distinct streams whose largest max_cnt exceeds krcnt. */
#define QH_ERR_QPACK_DECODER_STREAM_ERROR (-403) /* nghttp3.h:266 */
typedef struct qh_enc_ref { uint64_t stream_id, max_cnt, min_cnt, reserved; } qh_enc_ref;   /* 32 B */
typedef struct qh_enc_refs { uint64_t base, n, dlen, flags; } qh_enc_refs;                   /* 32 B */
#define QH_ENC_REFS_BAD 0x1u /* ctx.bad after a decoder-stream error */

QH_EXPORT void qh_enc_refs_init(qh_enc_refs *rv);

/* Before an encode: sec_flags[b] of section b on stream sec_sid[b], from the
 * state on entry (conn_start, nconns, tsel, ntables as qh_qpack_encode_conns
 * takes them): QH_ENC_SEC_STREAM_KNOWN iff a reference of the connection has
 * that stream id, QH_ENC_SEC_STREAM_BLOCKED iff moreover the largest max_cnt
 * of those references exceeds krcnt (:1165-1167).  status[c]: 0, or
 * QH_ERR_INVALID_ARGUMENT (and flags 0) for a connection that lists one
 * stream twice or whose rv region leaves refs[0, nrefs).  A table named
 * twice, or an index >= ntables: the call returns QH_ERR_INVALID_ARGUMENT.
 * The device call is asynchronous on the context stream, no host wait (the
 * table list is in HBM: a connection whose index is out of range, or whose
 * table another listed connection has claimed, gets status
 * QH_ERR_INVALID_ARGUMENT and flags 0 there instead). */
QH_EXPORT int qh_qpack_enc_sec_flags(
    const uint64_t *sec_sid, size_t nsections, const uint32_t *conn_start, size_t nconns,
    const uint32_t *tsel, size_t ntables, const qh_enc_state *enc, const qh_enc_refs *rv,
    const qh_enc_ref *refs, uint64_t nrefs, uint8_t *sec_flags, int32_t *status);
QH_EXPORT int qh_enc_sec_flags_batch(
    qh_ctx *ctx, const uint64_t *sec_sid, size_t nsections, const uint32_t *conn_start,
    size_t nconns, const uint32_t *tsel, size_t ntables, const qh_enc_state *enc,
    const qh_enc_refs *rv, const qh_enc_ref *refs, uint64_t nrefs, uint8_t *sec_flags,
    int32_t *status, int where);

/* After an encode, with its max_cnt, min_cnt and status: a listed connection
 * whose encode status is 0 gets dlen = 0 when it has at least one section
 * (:1186) and, unless enc has QH_ENC_IMMEDIATE_ACK, one reference {sid,
 * max_cnt, min_cnt, 0} per section with max_cnt > 0, in section order
 * (:1188-1194); it then moves as the layout rule says.  enc is only read
 * (the encode call has moved its scalars).  A table list error or an rv
 * region outside refs[0, *nrefs): QH_ERR_INVALID_ARGUMENT, nothing written.
 * The device call: a count pass, a scan, a flat copy over output records, one
 * host wait (the total against refs_cap). */
QH_EXPORT int qh_qpack_enc_refs_record(
    const uint64_t *sec_sid, size_t nsections, const uint32_t *conn_start, size_t nconns,
    const uint32_t *tsel, size_t ntables, const uint64_t *max_cnt, const uint64_t *min_cnt,
    const int32_t *enc_status, const qh_enc_state *enc, qh_enc_refs *rv, qh_enc_ref *refs,
    uint64_t *nrefs, uint64_t refs_cap);
QH_EXPORT int qh_enc_refs_record_batch(
    qh_ctx *ctx, const uint64_t *sec_sid, size_t nsections, const uint32_t *conn_start,
    size_t nconns, const uint32_t *tsel, size_t ntables, const uint64_t *max_cnt,
    const uint64_t *min_cnt, const int32_t *enc_status, const qh_enc_state *enc, qh_enc_refs *rv,
    qh_enc_ref *refs, uint64_t *nrefs, uint64_t refs_cap, int where);

/* The references of the listed connections (tsel NULL: all ntables, in
 * order) copied to refs_out[0, *nrefs_out), rv[].base rewritten.  On
 * QH_ERR_NOMEM *nrefs_out is the need and rv is untouched. */
QH_EXPORT int qh_qpack_enc_refs_compact(
    const uint32_t *tsel, size_t nconns, size_t ntables, qh_enc_refs *rv, const qh_enc_ref *refs,
    uint64_t nrefs, qh_enc_ref *refs_out, uint64_t *nrefs_out, uint64_t refs_out_cap);
QH_EXPORT int qh_enc_refs_compact_batch(
    qh_ctx *ctx, const uint32_t *tsel, size_t nconns, size_t ntables, qh_enc_refs *rv,
    const qh_enc_ref *refs, uint64_t nrefs, qh_enc_ref *refs_out, uint64_t *nrefs_out,
    uint64_t refs_out_cap, int where);

/* Decoder streams read: stream p is src[streams[p].off, + len) for
 * connection tsel[p] (NULL: p), the conventions those of
 * qh_qpack_dtables_apply: instructions applied in order, a trailing partial
 * instruction not consumed (hand the rest in again with what follows), the
 * first failing instruction sets status[p], the ones before it stay applied
 * and consumed[p] ends before it.  views is read for insert_count.
 * Per stream: QH_ENC_REFS_BAD set gives QH_ERR_QPACK_FATAL, nothing consumed
 * (:2553); length 0 gives 0; dlen + len > 4096 gives -403, nothing consumed,
 * dlen += len and BAD not set (:2561-2564 returns without marking the
 * context: the condition lasts until the next encode resets dlen); else dlen
 * += consumed.  Opcodes (:2571-2589): 1xxxxxxx Section Acknowledgment, 7-bit
 * prefix; 01xxxxxx Stream Cancellation, 6-bit; 00xxxxxx Insert Count
 * Increment, 6-bit; an integer overflow gives -403 and BAD.
 * Increment n: -403 and BAD when n == 0 or insert_count - krcnt < n, else
 * krcnt += n.  Acknowledgment sid: -403 and BAD when the connection has no
 * reference of that stream, else its oldest one is removed and krcnt =
 * max(krcnt, its max_cnt).  Cancellation sid: every reference of the stream
 * is removed; an unknown stream is no error.  Then pin_min, nstreams and
 * nblocked are recomputed.  A stream whose rv region leaves refs[0, nrefs)
 * gets QH_ERR_INVALID_ARGUMENT and is not touched.  A table named twice, or
 * an index >= ntables: the host call returns QH_ERR_INVALID_ARGUMENT and
 * nothing is written.  The device call (a 16-lane group per stream) is
 * asynchronous, no host wait: nothing grows; its table list is in HBM, so a
 * stream whose index is out of range, or whose table another listed stream
 * has claimed, gets status QH_ERR_INVALID_ARGUMENT there and is not applied. */
QH_EXPORT int qh_qpack_enc_read_decoder(
    const uint8_t *src, const qh_span_in *streams, const uint32_t *tsel, size_t nsel,
    size_t ntables, const qh_dtable_view *views, qh_enc_state *enc, qh_enc_refs *rv,
    qh_enc_ref *refs, uint64_t nrefs, int32_t *status, uint32_t *consumed);
QH_EXPORT int qh_enc_read_decoder_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *streams, const uint32_t *tsel, size_t nsel,
    size_t ntables, const qh_dtable_view *views, qh_enc_state *enc, qh_enc_refs *rv,
    qh_enc_ref *refs, uint64_t nrefs, int32_t *status, uint32_t *consumed, int where);

/* Decoder streams written, from a finished qh_emit_fields_batch: per emitted
 * block its stream id block_sid[], its table block_view[] and status[] /
 * ricnt[] as emit wrote them; cancel_sid[] / cancel_view[]: cancelled
 * streams; views for insert_count; written_icnt[ntables] in/out.  The blocks
 * of one table must be consecutive in the list, and so its cancellations
 * (else QH_ERR_INVALID_ARGUMENT, as for a table index >= ntables).
 * dstreams[t] is table t's span of dst (tables in index order, back to back,
 * length 0 when nothing is written), in this order:
 *   1. a Section Acknowledgment (0x80, 7-bit prefix) per block with status 0
 *      and ricnt > 0, in list order, written_icnt = max(written_icnt, ricnt);
 *   2. a Stream Cancellation (0x40, 6-bit prefix) per listed stream;
 *   3. if written_icnt < insert_count an Insert Count Increment (0x00, 6-bit)
 *      of the difference, written_icnt = insert_count.
 * The reference writes acknowledgements and cancellations in call order and
 * the increment last; this fixed order is the batch's definition (a caller
 * that needs another splits the call).  QH_ERR_NOMEM with *dst_need exact
 * when dst_cap is short; written_icnt is then untouched.  The reference's
 * limit on its internal buffer (qpack_decoder_dbuf_overflow) is not
 * restated: the caller owns dst.  The device call: a size pass, scans, a
 * write pass, one host wait for the total. */
QH_EXPORT int qh_qpack_dec_write_decoder(
    const uint64_t *block_sid, const uint32_t *block_view, const int32_t *status,
    const uint64_t *ricnt, size_t nblocks, const uint64_t *cancel_sid, const uint32_t *cancel_view,
    size_t ncancel, const qh_dtable_view *views, size_t ntables, uint64_t *written_icnt,
    uint8_t *dst, uint64_t dst_cap, qh_span_in *dstreams, uint64_t *dst_need);
QH_EXPORT int qh_dec_write_decoder_batch(
    qh_ctx *ctx, const uint64_t *block_sid, const uint32_t *block_view, const int32_t *status,
    const uint64_t *ricnt, size_t nblocks, const uint64_t *cancel_sid, const uint32_t *cancel_view,
    size_t ncancel, const qh_dtable_view *views, size_t ntables, uint64_t *written_icnt,
    uint8_t *dst, uint64_t dst_cap, qh_span_in *dstreams, uint64_t *dst_need, int where);

/* ---- Blocked field sections: queued, released and cancelled per batch ----
 *
 * What a decoder keeps for the sections qh_emit_fields_batch found blocked
 * (QH_EMIT_BLOCKED): which stream waits, for which table, at which Required
 * Insert Count, and the section's bytes -- the reference's per-connection
 * priority queue (lib/nghttp3_conn.c:263-271, :1463-1479, :1355, the limit
 * :1892-1895; examples/qpack_decode.cc:99-174) for many connections, with no
 * library object.  Table t's blocked sections are blks[bq[t].base, + bq[t].n)
 * in arrival order, in one caller-owned log blks[0, *nblks); their bytes are
 * pend[off, + len) in one caller-owned, append-only byte log pend[0, *npend).
 * bq[] lies beside views and acct.  Layout rules, the same on host and
 * device, so that both write the same bytes:
 *   - a table that gains a record in a call moves: its records are copied in
 *     order to the cursor and the new ones follow in list order; the cursor
 *     starts at *nblks and moves past each moved table in order of first
 *     appearance in the call's list;
 *   - removal never moves a table: its region is compacted in place, order
 *     kept, n shrinks (the records past the new n are left as they are);
 *   - new bytes go to pend at the byte cursor (*npend on entry), back to
 *     back in the order of the new records; older bytes are never moved;
 *   - when a capacity is short the call returns QH_ERR_NOMEM with the exact
 *     needs in *nblks / *npend (or the call's own need words) and nothing
 *     else written.
 * Each call has a host form over host pointers and a device form over
 * pointers in HBM (where must be QH_WHERE_DEVICE; counts are host scalars),
 * asynchronous on the context stream after the host wait named below.
 *
 * push, after an emit: every array is indexed by position in the emit
 * call's sel (src and blocks: the sections call's spans of the selected
 * blocks).  The blocks of one table must be consecutive; a second run of a
 * table or an index >= ntables gives QH_ERR_INVALID_ARGUMENT, nothing
 * written.  Per table the positions with status == QH_EMIT_BLOCKED are
 * examined in list order:
 *   1. the stream id is queued for the table, or was accepted earlier in the
 *      call: verdict QH_ERR_INVALID_ARGUMENT, not queued (a blocked stream
 *      delivers nothing further in the reference: a caller error);
 *   2. else n + the records accepted so far >= max_blocked: verdict
 *      QH_ERR_QPACK_DECOMPRESSION_FAILED, not queued (conn.c:1892-1895);
 *   3. else queued as {sid, ricnt, off, len}, its bytes copied, verdict
 *      QH_EMIT_BLOCKED.
 * Every other position gets verdict = status.  src needs no padding: nothing
 * is read outside src[blocks[p].off, + len).  Device: runs, a count pass (a
 * 16-lane group per table), one scan, one host wait (the totals and the
 * list's errors), then the verdicts, the record copy, the byte copy and the
 * rebase.
 *
 * release, after an apply: for each listed table (tsel, each at most once;
 * NULL: all, nsel = ntables) every record with ricnt <= views[t].insert_count
 * is removed and written to positions [rel_start[i], rel_start[i + 1]) of
 * rel_blocks (spans of pend), rel_sid, rel_view and rel_ricnt, ordered by
 * ascending ricnt, then queue position (the reference's (ricnt, seq) order);
 * the rest is compacted in place.  The outputs go as they are, with src =
 * pend, into qh_decode_sections_batch (blocks), qh_emit_fields_batch
 * (block_view) and qh_dec_write_decoder_batch (block_sid, block_view).
 * QH_ERR_NOMEM when rel_cap is short (*nreleased the need, nothing changed);
 * QH_ERR_INVALID_ARGUMENT for a table named twice or out of range.  Device:
 * a count pass, a scan, one host wait, a write pass (a group per table).
 *
 * cancel: the queued record of stream cancel_sid[i] of table cancel_view[i],
 * if there is one, is removed in place; removed[i] = 1 when one was (an
 * unknown stream is no error, qpack.c:3889-3913).  A table's cancellations
 * are consecutive.  The host form refuses a second run of a table or an index
 * out of range (QH_ERR_INVALID_ARGUMENT, nothing written); the device form
 * has no host wait and cannot: there the first run of a table is served and
 * the items of a later run, or of a table out of range, get removed[i] =
 * 0xFF and remove nothing.
 *
 * compact: the records of the listed tables copied to blks_out back to back
 * in list order, their bytes to pend_out in record order, off rewritten and
 * bq[].base rebased; QH_ERR_NOMEM with *nblks_out / *npend_out exact when a
 * capacity is short (nothing written); a record whose bytes lie outside
 * pend[0, npend) gives QH_ERR_INVALID_ARGUMENT.  When to compact is the
 * caller's decision.  Device: a count pass, a scan, one host wait, the
 * record copy, the byte copy, the rebase.
 *
 * Not built: emission with a given Required Insert Count.  A released block
 * is emitted like any other, so its Required Insert Count is reconstructed
 * again against the table's newer state, where the reference keeps the first
 * value; for a conformant encoder the two agree (a referenced entry is still
 * live).  rel_ricnt hands the queued value back so that a caller can compare. */
typedef struct qh_dec_blk  { uint64_t stream_id, ricnt, off; uint32_t len, reserved; } qh_dec_blk;  /* 32 B */
typedef struct qh_dec_blks { uint64_t base, n, max_blocked, flags; } qh_dec_blks;                  /* 32 B */
QH_EXPORT void qh_dec_blks_init(uint64_t max_blocked, qh_dec_blks *bq);

QH_EXPORT int qh_qpack_dec_blocked_push(
    const uint8_t *src, const qh_span_in *blocks, const uint64_t *block_sid,
    const uint32_t *block_view, const int32_t *status, const uint64_t *ricnt, size_t nblocks,
    size_t ntables, qh_dec_blks *bq, qh_dec_blk *blks, uint64_t *nblks, uint64_t blks_cap,
    uint8_t *pend, uint64_t *npend, uint64_t pend_cap, int32_t *verdict);
QH_EXPORT int qh_dec_blocked_push_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *blocks, const uint64_t *block_sid,
    const uint32_t *block_view, const int32_t *status, const uint64_t *ricnt, size_t nblocks,
    size_t ntables, qh_dec_blks *bq, qh_dec_blk *blks, uint64_t *nblks, uint64_t blks_cap,
    uint8_t *pend, uint64_t *npend, uint64_t pend_cap, int32_t *verdict, int where);

QH_EXPORT int qh_qpack_dec_blocked_release(
    const uint32_t *tsel, size_t nsel, size_t ntables, const qh_dtable_view *views,
    qh_dec_blks *bq, qh_dec_blk *blks, uint64_t nblks, qh_span_in *rel_blocks, uint64_t *rel_sid,
    uint32_t *rel_view, uint64_t *rel_ricnt, uint32_t *rel_start, uint64_t *nreleased,
    uint64_t rel_cap);
QH_EXPORT int qh_dec_blocked_release_batch(
    qh_ctx *ctx, const uint32_t *tsel, size_t nsel, size_t ntables, const qh_dtable_view *views,
    qh_dec_blks *bq, qh_dec_blk *blks, uint64_t nblks, qh_span_in *rel_blocks, uint64_t *rel_sid,
    uint32_t *rel_view, uint64_t *rel_ricnt, uint32_t *rel_start, uint64_t *nreleased,
    uint64_t rel_cap, int where);

QH_EXPORT int qh_qpack_dec_blocked_cancel(
    const uint64_t *cancel_sid, const uint32_t *cancel_view, size_t ncancel, size_t ntables,
    qh_dec_blks *bq, qh_dec_blk *blks, uint64_t nblks, uint8_t *removed);
QH_EXPORT int qh_dec_blocked_cancel_batch(
    qh_ctx *ctx, const uint64_t *cancel_sid, const uint32_t *cancel_view, size_t ncancel,
    size_t ntables, qh_dec_blks *bq, qh_dec_blk *blks, uint64_t nblks, uint8_t *removed,
    int where);

QH_EXPORT int qh_qpack_dec_blocked_compact(
    const uint32_t *tsel, size_t nsel, size_t ntables, qh_dec_blks *bq, const qh_dec_blk *blks,
    uint64_t nblks, const uint8_t *pend, uint64_t npend, qh_dec_blk *blks_out, uint64_t *nblks_out,
    uint64_t blks_out_cap, uint8_t *pend_out, uint64_t *npend_out, uint64_t pend_out_cap);
QH_EXPORT int qh_dec_blocked_compact_batch(
    qh_ctx *ctx, const uint32_t *tsel, size_t nsel, size_t ntables, qh_dec_blks *bq,
    const qh_dec_blk *blks, uint64_t nblks, const uint8_t *pend, uint64_t npend,
    qh_dec_blk *blks_out, uint64_t *nblks_out, uint64_t blks_out_cap, uint8_t *pend_out,
    uint64_t *npend_out, uint64_t pend_out_cap, int where);

/* ---- Field sections in pieces: reassembled per batch ----------------------
 *
 * Every decoder call above takes complete field sections.  The reference
 * reads a request stream as it arrives: nghttp3_conn hands
 * nghttp3_qpack_decoder_read_request whatever part of a HEADERS frame is there,
 * fin = 0 until the last part (lib/nghttp3_conn.c:1880-1883), the stream
 * context keeps the parse between calls (lib/nghttp3_qpack.c:3347-3805).  Here
 * a section's bytes are held until its last piece arrives and are then decoded
 * whole, by the calls above; nothing is parsed before.  Table t's unfinished
 * sections are parts[pq[t].base, + pq[t].n), in the order their first pieces
 * arrived, in one caller-owned log parts[0, *nparts); a section's bytes so far
 * are held[off, + len), contiguous, in one caller-owned, append-only byte log
 * held[0, *nheld).  pq[] lies beside views, acct and bq.  Each call has a host
 * form over host pointers and a device form over pointers in HBM (where must
 * be QH_WHERE_DEVICE; counts are host scalars), asynchronous on the context
 * stream after its one host wait.
 *
 * push: piece p is src[pieces[p].off, + len) of stream piece_sid[p] of table
 * piece_view[p]; piece_fin[p] != 0: the section ends with it.  The pieces of
 * one table must be consecutive; a second run of a table or an index >=
 * ntables gives QH_ERR_INVALID_ARGUMENT, nothing written.  Per table the
 * pieces are examined in list order:
 *   1. the stream id appeared earlier in the table's run: verdict
 *      QH_ERR_INVALID_ARGUMENT, the piece is ignored and the earlier one
 *      stands (a caller joins what it received for one stream before the
 *      call, as its QUIC stream buffer already does);
 *   2. else the held length + the piece's length > max_bytes: verdict
 *      QH_ERR_QPACK_HEADER_TOO_LARGE, the stream's record, if it has one, is
 *      removed, nothing is kept or handed on.  The limit is this project's
 *      own (and at most 2^32 - 1): it stands where nghttp3_conn bounds a
 *      HEADERS frame by its announced length before a byte reaches QPACK;
 *   3. else fin: verdict QH_PART_DONE, the held bytes followed by the piece
 *      are written to done at its cursor, the record is removed.  A section
 *      that arrives whole takes this path with nothing held; an empty result
 *      is handed on as an empty block, to which the sections call gives the
 *      status it gives any empty block;
 *   4. else verdict QH_PART_KEPT.  A piece of length 0 changes nothing (and
 *      makes no record).  Otherwise the record's old bytes followed by the
 *      piece are written at the byte cursor of held and off / len are
 *      rewritten (no reserved room, no append in place); a stream without a
 *      record gains one.
 * Finished section j (in list order of the fin pieces) is done[done_blocks[j]
 * .off, + len) of stream done_sid[j] of table done_view[j]; the three arrays
 * have room for npieces entries, *ndone is their count, *done_need the bytes.
 * They go as they are into qh_decode_sections_batch (src = done, blocks =
 * done_blocks), qh_emit_fields_batch (block_view), qh_dec_write_decoder_batch
 * and qh_dec_blocked_push_batch (block_sid, block_view, src = done).  Layout
 * rules, the same on host and device, so that both logs are equal byte for
 * byte, dead regions included:
 *   - a table that gains a record moves: its surviving records (off / len as
 *     rewritten) are copied in order to the record cursor, the new ones
 *     follow in list order, the old region is left as it was; the cursor
 *     starts at *nparts and passes each moved table in order of first
 *     appearance in the list;
 *   - a table that only loses records, or whose records only change off /
 *     len, is compacted in place, order kept (the records past the new n are
 *     left as they are);
 *   - new held bytes go back to back in list order of the pieces that cause
 *     them, older bytes are never touched; done is filled back to back;
 *   - when a capacity is short the call returns QH_ERR_NOMEM with the exact
 *     needs in *nparts, *nheld, *done_need and *ndone and nothing else
 *     written;
 *   - nothing is read outside src[pieces[p].off, + len): src needs no padding.
 * A record whose bytes are needed and lie outside held[0, *nheld) gives
 * QH_ERR_INVALID_ARGUMENT.  done must not overlap held.  Device: runs, a count
 * pass (a 16-lane group per table), one scan over four segments, one host
 * wait (the totals and the list's errors), then verdicts and copy items, the
 * byte copies (two sources per output section: the old bytes, then the
 * piece), the records.
 *
 * cancel (a stream reset): exactly qh_dec_blocked_cancel's semantics, host and
 * device (0xFF for a later run on the device).  nghttp3_qpack_decoder_
 * cancel_stream has no held bytes to drop; here there are some.
 *
 * compact: as qh_dec_blocked_compact.  Every continued section leaves its
 * previous copy dead in held, so this log wants compacting more often than
 * the blocked one: after k continuations of a section of n bytes about k n / 2
 * bytes are dead.
 *
 * Not built: the reference reports a framing error at the piece where it
 * occurs and BLOCKED as soon as the two prefix integers are read; here both
 * come at fin, from the whole-section calls (the final verdict, fields,
 * Required Insert Count and decoder-stream bytes are the same).  A limit on
 * open streams per table (the caller's QUIC stream limit bounds it),
 * QH_WHERE_HOST staging, a hashed stream index. */
#define QH_PART_DONE 0 /* verdict: the section is complete and in done */
#define QH_PART_KEPT 2 /* verdict: the piece is held (or was empty)    */
typedef struct qh_dec_part  { uint64_t stream_id, off; uint32_t len, reserved0; uint64_t reserved1; } qh_dec_part;   /* 32 B */
typedef struct qh_dec_parts { uint64_t base, n, max_bytes, flags; } qh_dec_parts;                                    /* 32 B */
QH_EXPORT void qh_dec_parts_init(uint64_t max_bytes, qh_dec_parts *pq);

QH_EXPORT int qh_qpack_dec_partial_push(
    const uint8_t *src, const qh_span_in *pieces, const uint64_t *piece_sid,
    const uint32_t *piece_view, const uint8_t *piece_fin, size_t npieces, size_t ntables,
    qh_dec_parts *pq, qh_dec_part *parts, uint64_t *nparts, uint64_t parts_cap, uint8_t *held,
    uint64_t *nheld, uint64_t held_cap, int32_t *verdict, uint8_t *done, uint64_t done_cap,
    uint64_t *done_need, qh_span_in *done_blocks, uint64_t *done_sid, uint32_t *done_view,
    uint64_t *ndone);
QH_EXPORT int qh_dec_partial_push_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *pieces, const uint64_t *piece_sid,
    const uint32_t *piece_view, const uint8_t *piece_fin, size_t npieces, size_t ntables,
    qh_dec_parts *pq, qh_dec_part *parts, uint64_t *nparts, uint64_t parts_cap, uint8_t *held,
    uint64_t *nheld, uint64_t held_cap, int32_t *verdict, uint8_t *done, uint64_t done_cap,
    uint64_t *done_need, qh_span_in *done_blocks, uint64_t *done_sid, uint32_t *done_view,
    uint64_t *ndone, int where);

QH_EXPORT int qh_qpack_dec_partial_cancel(
    const uint64_t *cancel_sid, const uint32_t *cancel_view, size_t ncancel, size_t ntables,
    qh_dec_parts *pq, qh_dec_part *parts, uint64_t nparts, uint8_t *removed);
QH_EXPORT int qh_dec_partial_cancel_batch(
    qh_ctx *ctx, const uint64_t *cancel_sid, const uint32_t *cancel_view, size_t ncancel,
    size_t ntables, qh_dec_parts *pq, qh_dec_part *parts, uint64_t nparts, uint8_t *removed,
    int where);

QH_EXPORT int qh_qpack_dec_partial_compact(
    const uint32_t *tsel, size_t nsel, size_t ntables, qh_dec_parts *pq, const qh_dec_part *parts,
    uint64_t nparts, const uint8_t *held, uint64_t nheld, qh_dec_part *parts_out,
    uint64_t *nparts_out, uint64_t parts_out_cap, uint8_t *held_out, uint64_t *nheld_out,
    uint64_t held_out_cap);
QH_EXPORT int qh_dec_partial_compact_batch(
    qh_ctx *ctx, const uint32_t *tsel, size_t nsel, size_t ntables, qh_dec_parts *pq,
    const qh_dec_part *parts, uint64_t nparts, const uint8_t *held, uint64_t nheld,
    qh_dec_part *parts_out, uint64_t *nparts_out, uint64_t parts_out_cap, uint8_t *held_out,
    uint64_t *nheld_out, uint64_t held_out_cap, int where);

/* ---- Encoder and decoder streams as they arrive: cut instructions held ----
 *
 * qh_dtables_apply_batch and qh_enc_read_decoder_batch stop before an
 * instruction that the end of the input cuts and leave the rest to the caller.
 * The reference takes whatever has arrived and buffers a cut instruction
 * itself (nghttp3_qpack_decoder_read_encoder lib/nghttp3_qpack.c:2815-3157,
 * nghttp3_qpack_encoder_read_decoder :2545-2641).  This layer keeps that tail
 * beside the other per-connection records: one qh_ustream per table (beside
 * views / acct / bq / pq) or per connection (beside qh_enc_refs), the unread
 * bytes log[off, + len) in one caller-owned, append-only byte log
 * log[0, *nlog).  Each call has a host form over host pointers and a device
 * form over pointers in HBM (where must be QH_WHERE_DEVICE; counts are host
 * scalars).  The host functions and the kernels compile the same rules
 * (csrc/qh_ustream_core.h) and follow the same layout, so records, log (dead
 * regions included), joined and verdicts are equal byte for byte.
 *
 * A record also holds the two pieces of read_encoder's per-connection state
 * that no other call keeps: flags & QH_USTREAM_BAD is decoder->ctx.bad (set at
 * :3155 after an encoder-stream error and at :3803 after a failed section,
 * tested at :2826), ulen is uninterrupted_encoderlen (:2834-2837, limited by
 * NGHTTP3_QPACK_MAX_ENCODERLEN = 131,072, lib/nghttp3_qpack.h:54; reset when a
 * section finishes, :3797).  The encoder side's 4 KiB twin is
 * qh_enc_refs.dlen, kept by qh_enc_read_decoder_batch itself.
 *
 * join: piece p is src[pieces[p].off, + len), the new bytes of the stream of
 * table tsel[p] (NULL: table p, nsel = ntables).  limit is
 * QH_USTREAM_MAX_ENCODERLEN for tables and 0 (no rule) for decoder streams.
 * Per listed stream, in list order:
 *   1. QH_USTREAM_BAD set: verdict QH_ERR_QPACK_FATAL (-108), the piece is
 *      dropped, joined[p] is empty, the record is unchanged;
 *   2. else an empty piece: verdict 0, joined[p] is the tail as it lies
 *      (off, len), held = len, no byte is copied;
 *   3. else limit != 0 and ulen + len > limit: verdict
 *      QH_ERR_QPACK_ENCODER_STREAM_ERROR (-402), ulen += len all the same (as
 *      :2834), BAD is not set, the piece is dropped, the tail is kept,
 *      joined[p] is empty;
 *   4. else verdict 0: the tail followed by the piece is written at the log's
 *      cursor, held = the old len, off = the cursor, len += the piece's, (limit
 *      != 0) ulen += the piece's, joined[p] = (off, len).
 * An empty joined[p] is (0, 0).  joined goes as it is into
 * qh_dtables_apply_batch / qh_enc_read_decoder_batch as `streams`, with src =
 * log and the same list; the call's status for p is verdict[p] where that is
 * negative, else the apply's or read's.  New bytes go back to back in list
 * order at *nlog; nothing written earlier is modified, and the tail of a table
 * that is not listed stays where it is.  Nothing is read outside a piece or a
 * tail.  Returns 0; QH_ERR_INVALID_ARGUMENT with nothing written when a table
 * index is >= ntables, a table is named twice, a listed record's tail leaves
 * log[0, *nlog) or tail + piece is 2^32 bytes or more; QH_ERR_NOMEM when
 * log_cap is short, *nlog then the exact need and nothing else written.
 * Device: a lane per stream (rules and lengths), one qh_k_scan_seg, one host
 * wait for the total and the error flag, a lane per stream (records, joined,
 * verdicts, two copy items per stream: the tail, then the piece), the byte
 * copy of the pieces layer (qh_k_part_bytes: a lane per 16 bytes of the
 * destination, so one long tail and many short ones balance).
 *
 * keep: after the apply or read, with its status and consumed and the same
 * list.  status 0: off += consumed, len -= consumed (consumed above len counts
 * as len).  status < 0 with QH_USTREAM_LATCH (tables): len = 0 and BAD is set.
 * status < 0 without it (decoder streams): len = min(len, held): a refused
 * call read nothing (:2553-2564), so the head the reference buffered before it
 * survives; after an error that sets QH_ENC_REFS_BAD nothing is read again.
 * No bytes move; the device call is asynchronous and has no host wait, so a
 * list error (which the join before it has already refused) leaves the
 * offending streams untouched there and is QH_ERR_INVALID_ARGUMENT with
 * nothing written on the host.  An apply that answers QH_ERR_NOMEM is repeated
 * on the same joined before keep.
 *
 * sections: after a finished emit call, with its status per block and
 * block_view (NULL: table 0).  A table with a block of status 0 gets ulen = 0
 * (:3797); one with a block of status < 0 gets BAD (:3803); QH_EMIT_BLOCKED
 * changes nothing.  Host: a block_view entry >= ntables is
 * QH_ERR_INVALID_ARGUMENT, nothing written; device (a lane per block, no host
 * wait): such a block is passed over.
 *
 * compact: the tails of all ntables records copied back to back, in table
 * order, to a fresh log (log_out, not overlapping log), off rebased (an empty
 * tail's too); len, held, ulen and flags stay.  log_out_cap 0 with a null
 * log_out is the sizing call: QH_ERR_NOMEM, *nlog_out the exact need, records
 * untouched.  A tail that leaves log[0, nlog) is QH_ERR_INVALID_ARGUMENT,
 * nothing written.  Call it between a keep and the next join (held describes
 * the last joined stream, which is gone).  Every join writes tail + piece
 * anew, so the log grows by what arrives plus the tails; a caller may compact
 * after every keep at the cost of the tails alone, and no tail is longer than
 * the longest instruction the scanners accept (an encoder-stream insert of
 * 10 + 256 + 10 + 65,536 bytes, a decoder-stream instruction of 11).
 *
 * Not built: the reference parses byte by byte and may report an error inside
 * an instruction that is still cut (in the recorded cases: a dynamic name
 * index that is not live while the value is still to come); here the apply
 * sees whole instructions, so the same code comes at the call that delivers
 * the instruction's last byte, status 0 until then (the reference's is the
 * error and then -108), the table states equal at every step, and no
 * instruction the reference did not apply is applied.
 * On the decoder stream the read is handed tail and piece, so dlen takes the
 * tail with the piece that completes it; the reference counted the head when
 * it came.  Where a tail is held while an encode resets dlen, or while a call
 * is refused by the length rule (-403), the next call that is read counts the
 * head once more: until the next encode with no tail held dlen is ahead of the
 * reference's count by at most a cut instruction's bytes, and a piece that
 * takes the reference's count into (4096 - tail, 4096] is refused here where
 * the reference still accepts it.  QH_WHERE_HOST staging, a
 * per-table selection for compact. */
#define QH_USTREAM_BAD 0x1u           /* qh_ustream.flags: ctx.bad, nothing is read again */
#define QH_USTREAM_LATCH 0x1u         /* keep opts: a failed stream sets QH_USTREAM_BAD   */
#define QH_USTREAM_MAX_ENCODERLEN 131072u /* NGHTTP3_QPACK_MAX_ENCODERLEN */
typedef struct qh_ustream { /* 32 B */
  uint64_t off;  /* the unread bytes are log[off, + len)                          */
  uint32_t len;
  uint32_t held; /* of the last joined stream, the leading bytes that were tail   */
  uint64_t ulen; /* uninterrupted_encoderlen                                      */
  uint32_t flags;
  uint32_t reserved;
} qh_ustream;
QH_EXPORT void qh_ustream_init(qh_ustream *us);

QH_EXPORT int qh_qpack_ustream_join(
    const uint8_t *src, const qh_span_in *pieces, const uint32_t *tsel, size_t nsel, size_t ntables,
    uint64_t limit, qh_ustream *us, uint8_t *log, uint64_t *nlog, uint64_t log_cap,
    qh_span_in *joined, int32_t *verdict);
QH_EXPORT int qh_ustream_join_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *pieces, const uint32_t *tsel, size_t nsel,
    size_t ntables, uint64_t limit, qh_ustream *us, uint8_t *log, uint64_t *nlog, uint64_t log_cap,
    qh_span_in *joined, int32_t *verdict, int where);

QH_EXPORT int qh_qpack_ustream_keep(
    const int32_t *status, const uint32_t *consumed, const uint32_t *tsel, size_t nsel,
    size_t ntables, uint32_t opts, qh_ustream *us);
QH_EXPORT int qh_ustream_keep_batch(
    qh_ctx *ctx, const int32_t *status, const uint32_t *consumed, const uint32_t *tsel, size_t nsel,
    size_t ntables, uint32_t opts, qh_ustream *us, int where);

QH_EXPORT int qh_qpack_ustream_sections(
    const int32_t *status, const uint32_t *block_view, size_t nblocks, size_t ntables,
    qh_ustream *us);
QH_EXPORT int qh_ustream_sections_batch(
    qh_ctx *ctx, const int32_t *status, const uint32_t *block_view, size_t nblocks, size_t ntables,
    qh_ustream *us, int where);

QH_EXPORT int qh_qpack_ustream_compact(
    size_t ntables, qh_ustream *us, const uint8_t *log, uint64_t nlog, uint8_t *log_out,
    uint64_t *nlog_out, uint64_t log_out_cap);
QH_EXPORT int qh_ustream_compact_batch(
    qh_ctx *ctx, size_t ntables, qh_ustream *us, const uint8_t *log, uint64_t nlog,
    uint8_t *log_out, uint64_t *nlog_out, uint64_t log_out_cap, int where);

/* ---- Decoded header sections as HTTP messages --------
 * What conn_decode_headers does with every emitted field
 * (lib/nghttp3_conn.c:1880-1944): nghttp3_http_on_header
 * (lib/nghttp3_http.c:538-571, the two switches :319-534) passes it on, drops
 * it (NGHTTP3_ERR_REMOVE_HTTP_HEADER) or fails the stream
 * (NGHTTP3_ERR_MALFORMED_HTTP_HEADER), and the end of a header section is
 * nghttp3_http_on_request_headers / _on_response_headers (http.c:573-627,
 * conn.c:1713-1730), for every section of a batch.
 *
 * Inputs: the outputs of an emit call made with `out` -- fields (nfields
 * records), field_start (nsec + 1), out (nout bytes) and optionally emit's
 * status (emit_status, nsec) -- plus kind[p], one byte per section
 * (QH_HTTP_REQUEST or 0 for a response, | QH_HTTP_TRAILERS, |
 * QH_HTTP_CONNECT_PROTOCOL: conn->server && enable_connect_protocol,
 * conn.c:1917), and states[p], in / out: section p owns record p (the caller
 * gathers and scatters per-stream records, so the sections of a call are
 * independent).  The state carries what a later section of the stream needs:
 * the request's method for its response (METH_HEAD, METH_CONNECT;
 * nghttp3_http_record_request_method :651-673), EXPECT_FINAL_RESPONSE after
 * a 1xx, the headers' flags for the trailers.
 *
 * Outputs:
 *   fverdict[f]  QH_HTTP_KEEP, _REMOVE, _MALFORMED, or _UNSEEN for a field
 *                behind the section's first malformed one (the reference
 *                never reads it) and for every field of a skipped section;
 *   status[p]    0 or QH_ERR_MALFORMED_HTTP_HEADER;
 *   bad_field[p] (optional) the section-relative index of the malformed
 *                field, the section's field count when the end-of-headers
 *                check failed, QH_HTTP_NO_FIELD otherwise;
 *   kept, kept_start[nsec + 1] (optional, together) the records recv_header
 *                / recv_trailer would receive (conn.c:1924-1931), compacted
 *                in order: the KEEP fields before any malformed one, section
 *                p's at [kept_start[p], kept_start[p + 1]).  kept_cap >=
 *                nfields is required, so that nothing has to come back to the
 *                host;
 *   states[p]    updated when status[p] is 0.
 * A section is skipped (verdicts UNSEEN, nothing kept, state untouched) when
 * emit_status[p] != 0 (copied to status[p]), or when its range does not lie
 * inside [0, nfields) or one of its records does not have both strings in
 * out[0, nout) as QH_IN_OUT (status[p] = QH_ERR_INVALID_ARGUMENT).
 *
 * Two departures from the reference: (1) the `priority` dictionary
 * (http.c:437-449) is not parsed: a request's priority field with a bad
 * value byte is removed and sets QH_HTTP_FLAG_BAD_PRIORITY (:426-431),
 * otherwise it is kept and QH_HTTP_FLAG_PRIORITY is never set -- the caller
 * finds the field by its token; (2) the state of a section that ends -105 is
 * left as on entry (the reference leaves a partial state on a stream it then
 * resets).
 *
 * Returns 0, or QH_ERR_INVALID_ARGUMENT with nothing written (a NULL
 * argument that is needed, kept without kept_start or the reverse, kept_cap <
 * nfields, nfields or nsec of 2^31 or more).  qh_qpack_http_check is host C
 * over host pointers; qh_http_check_batch is the same over pointers in HBM
 * (where must be QH_WHERE_DEVICE), asynchronous on the context stream with
 * no host wait. */
#define QH_ERR_MALFORMED_HTTP_HEADER (-105) /* nghttp3.h:211 */

#define QH_HTTP_REQUEST 1u
#define QH_HTTP_TRAILERS 2u
#define QH_HTTP_CONNECT_PROTOCOL 4u

#define QH_HTTP_KEEP 0
#define QH_HTTP_REMOVE 1
#define QH_HTTP_MALFORMED 2
#define QH_HTTP_UNSEEN 3
#define QH_HTTP_NO_FIELD 0xFFFFFFFFu

/* NGHTTP3_HTTP_FLAG_*, lib/nghttp3_http.h:42-83 */
#define QH_HTTP_FLAG__AUTHORITY 0x01u
#define QH_HTTP_FLAG__PATH 0x02u
#define QH_HTTP_FLAG__METHOD 0x04u
#define QH_HTTP_FLAG__SCHEME 0x08u
#define QH_HTTP_FLAG_HOST 0x10u
#define QH_HTTP_FLAG__STATUS 0x20u
#define QH_HTTP_FLAG_REQ_HEADERS \
  (QH_HTTP_FLAG__METHOD | QH_HTTP_FLAG__PATH | QH_HTTP_FLAG__SCHEME)
#define QH_HTTP_FLAG_PSEUDO_HEADER_DISALLOWED 0x40u
#define QH_HTTP_FLAG_METH_CONNECT 0x80u
#define QH_HTTP_FLAG_METH_HEAD 0x0100u
#define QH_HTTP_FLAG_METH_OPTIONS 0x0200u
#define QH_HTTP_FLAG_METH_ALL \
  (QH_HTTP_FLAG_METH_CONNECT | QH_HTTP_FLAG_METH_HEAD | QH_HTTP_FLAG_METH_OPTIONS)
#define QH_HTTP_FLAG_PATH_REGULAR 0x0400u
#define QH_HTTP_FLAG_PATH_ASTERISK 0x0800u
#define QH_HTTP_FLAG_SCHEME_HTTP 0x1000u
#define QH_HTTP_FLAG_EXPECT_FINAL_RESPONSE 0x2000u
#define QH_HTTP_FLAG__PROTOCOL 0x4000u
#define QH_HTTP_FLAG_PRIORITY 0x8000u
#define QH_HTTP_FLAG_BAD_PRIORITY 0x010000u

typedef struct qh_http_state { /* 16 B: nghttp3_http_state without pri and recv_content_length */
  int64_t content_length;
  int32_t status_code;
  uint32_t flags; /* QH_HTTP_FLAG_* */
} qh_http_state;
/* -1 / -1 / 0, as lib/nghttp3_stream.c:67-68 sets them. */
QH_EXPORT void qh_http_state_init(qh_http_state *states, size_t n);

QH_EXPORT int qh_qpack_http_check(
    const qh_field *fields, size_t nfields, const uint32_t *field_start, size_t nsec,
    const uint8_t *out, uint64_t nout, const int32_t *emit_status, const uint8_t *kind,
    qh_http_state *states, int8_t *fverdict, int32_t *status, uint32_t *bad_field,
    qh_field *kept, size_t kept_cap, uint32_t *kept_start);
QH_EXPORT int qh_http_check_batch(
    qh_ctx *ctx, const qh_field *fields, size_t nfields, const uint32_t *field_start,
    size_t nsec, const uint8_t *out, uint64_t nout, const int32_t *emit_status,
    const uint8_t *kind, qh_http_state *states, int8_t *fverdict, int32_t *status,
    uint32_t *bad_field, qh_field *kept, size_t kept_cap, uint32_t *kept_start, int where);

/* ---- Request streams as they arrive: HTTP/3 frames cut per batch ----------
 *
 * What nghttp3_conn_read_bidi does with the bytes of a request stream
 * (lib/nghttp3_conn.c:1514-1813): the frame type and length varints, which a
 * packet may cut anywhere (nghttp3_read_varint, lib/nghttp3_stream.c:181-223),
 * the HEADERS / DATA / unknown-frame state machine, which frames are legal
 * when (nghttp3_stream_transit_rx_http_state, stream.c:1057-1226) and the body
 * accounting against content-length (nghttp3_http_on_data_chunk and
 * nghttp3_http_on_remote_end_stream, lib/nghttp3_http.c:629-649), for the
 * chunks of many streams in one call.  Its output is the input of the pieces
 * layer (qh_dec_partial_push_batch) and of the HTTP check.  Each call has a
 * host form over host pointers and a device form over pointers in HBM (where
 * must be QH_WHERE_DEVICE; counts are host scalars); both compile the same
 * rules (csrc/qh_h3_core.h) and agree byte for byte on every output and
 * every record.
 *
 * qh_h3_stream is the per-stream record, beside the stream's qh_http_state
 * and caller-owned; chunk c owns rs[c] and hs[c] (the caller gathers and
 * scatters, as for the HTTP check).  Layout (32 B):
 *   left    rstate->left: payload bytes of the frame in progress still to
 *           come (up to 2^62 - 1);
 *   acc     rvint->acc: the value of the bytes of a cut varint read so far
 *           (the first byte's length bits removed);
 *   recv    recv_content_length;
 *   state   QH_H3_ST_* (NGHTTP3_REQ_STREAM_STATE_*, lib/nghttp3_stream.h:77-84);
 *   vleft   rvint->left: the bytes of the cut varint still missing (0 to 7);
 *   fclass  QH_H3_F_*: the class of the frame in progress (set once its type
 *           is read);
 *   hstate  the rx HTTP state (NGHTTP3_HTTP_STATE_*, stream.h:133-151: 1
 *           REQ_INITIAL .. 8 REQ_END, 9 RESP_INITIAL .. 16 RESP_END);
 *   flags   QH_H3_RESPONSE (a client reading responses: selects RESP_INITIAL),
 *           QH_H3_PENDING, QH_H3_SAW_DATA, QH_H3_SAW_END;
 *   err     the first error, latched (0: none).
 *
 * read.  Chunk c is src[chunks[c].off, + len), the new bytes of stream
 * chunk_sid[c] of table chunk_view[c], chunk_fin[c] != 0 when they end the
 * stream.  Per chunk:
 *   status[c]    QH_H3_OPEN, QH_H3_END, QH_H3_WAIT or the error;
 *   consumed[c]  the bytes of the chunk that were walked;
 *   nunknown[c]  (optional) the unknown frames begun (the reference's glitch
 *                rate limiter, conn.c:1657, is per connection and timed: the
 *                caller's).
 * HEADERS pieces, compacted in chunk order: pieces[j] (a span into src),
 * piece_sid, piece_view, piece_fin, piece_kind (QH_HTTP_REQUEST or 0, |
 * QH_HTTP_TRAILERS), *npieces.  The first four go as they are into
 * qh_dec_partial_push_batch, piece_kind (per finished section) to the HTTP
 * check.  A chunk yields at most one piece, so room for nchunks entries always
 * suffices and is required.  A piece exists only when at least one payload
 * byte of a HEADERS frame lies in the chunk and carries fin only when it holds
 * the frame's last byte.  Body spans: dspans[dspan_start[c], dspan_start[c +
 * 1]) are the spans into src that recv_data would receive for chunk c, in
 * order (dspan_start has nchunks + 1 entries).  When dspan_cap is short the
 * call returns QH_ERR_NOMEM with the exact need in *ndspans and nothing else
 * written.  Rules per chunk, in the reference's order:
 *   1. an error is latched: status is that error, consumed 0, nothing changes;
 *   2. QH_H3_PENDING is set: status QH_H3_WAIT, consumed 0, nothing changes and
 *      fin is not acted on (conn.c:1533-1545 buffers a stream whose headers are
 *      blocked); the caller feeds the same bytes again after the settle call;
 *   3. else the chunk is walked as read_bidi walks it.  Varints are continued
 *      from the record; one cut by fin is -606 in the type state and -602 in
 *      the length state.  DATA: the transition, recv += the bytes,
 *      on_data_chunk against hs[c], a span (an empty DATA frame makes its
 *      transitions and no span).  HEADERS: the transition with its three tests
 *      against hs[c] (METH_CONNECT; status_code == -1 after a 1xx; CONNECT
 *      with a 2xx); length 0 outside trailers is -107, empty trailers begin
 *      and end with no piece.  The eleven types of conn.c:1643-1653 are -601
 *      once their length is read; every other type is skipped and counted.
 *      fin at a frame boundary is MSG_END (on_remote_end_stream, status
 *      QH_H3_END), anywhere else -602; in QH_H3_ST_IGN_REST (set by qh_h3_dispatch_batch or the caller,
 *      conn.c:506) everything is consumed and fin ends nothing.
 *      The one departure: when a HEADERS frame that is not trailers ends, the
 *      record gains QH_H3_PENDING, because hs[c] does not know that section
 *      yet.  For the rest of the call DATA frames are taken provisionally
 *      (QH_H3_SAW_DATA, counted into recv, spans emitted), unknown frames are
 *      skipped, refused types are still -601, fin at a boundary sets
 *      QH_H3_SAW_END with status 0, and a HEADERS frame stops the walk as soon
 *      as its type is known: consumed[c] is the offset of that frame's first
 *      byte, the record is clean in the type state, status QH_H3_WAIT;
 *   4. on an error the record is left as on entry with the error latched,
 *      consumed[c] is the offset of the first byte of the frame at which it
 *      arose (0 when that lies in an earlier chunk), and the piece and spans
 *      of the chunk that precede it stay.
 * Returns 0; QH_ERR_INVALID_ARGUMENT with nothing written for a NULL argument
 * that is needed, nchunks of 2^27 or more, or a record that no call here
 * leaves (state, vleft, fclass, hstate or flags out of range); QH_ERR_NOMEM as
 * above.  No byte outside a chunk is read: src needs no padding.  Device: a
 * lane per chunk hops from frame header to frame header (payloads are not
 * read) and counts, one scan over two segments, one host wait (the totals and
 * the list's errors), then a lane per chunk replays the walk and writes.
 *
 * settle, after the HTTP check, for the streams whose section was checked:
 * rs[j], hs[j] (now including the section), sec_status[j] (the check's status;
 * NULL: all 0).  A record without QH_H3_PENDING is untouched, status 0.
 * sec_status[j] < 0 is latched and returned.  Otherwise what rule 3 deferred,
 * in stream order: (1) QH_H3_SAW_DATA with EXPECT_FINAL_RESPONSE is -601
 * (stream.c:1166); (2) content_length != -1 and recv > content_length is -107
 * (on_data_chunk); (3) QH_H3_SAW_END with EXPECT_FINAL_RESPONSE or a
 * content_length that differs from recv is -107 (on_remote_end_stream); (4)
 * else the three flags are cleared, status QH_H3_END and hstate *_END when
 * the end was seen, else 0.  An error is latched and leaves the rest of the
 * record as it was (a later settle of that record answers the same error).  The device form is asynchronous on the context stream,
 * with no host wait, and reads no stream bytes.
 *
 * A round is read -> partial push -> sections -> emit -> HTTP check ->
 * settle.  A stream with headers, body and fin in one chunk is finished in
 * that round; headers and trailers in one chunk, a 1xx and the final response
 * in one chunk, or a blocked section are fed their rest in the next.
 *
 * Departures: the body spans of a call are valid only once the settle answers
 * non-negative (the reference would have refused the overflowing chunk before
 * recv_data); -107 for a body is reported at settle, not at the byte where it
 * occurs; begin_headers / end_headers with fin have no output; the caller's
 * QUIC stream buffer holds the tail after QH_H3_WAIT (consumed says where it
 * begins).  Not built: `priority`, QH_WHERE_HOST staging, a tail log as qh_ustream_* keeps.  (Frame writing is
 * the next section.) */
#define QH_ERR_MALFORMED_HTTP_MESSAGING (-107)   /* nghttp3.h:210 */
#define QH_ERR_H3_FRAME_UNEXPECTED (-601)        /* nghttp3.h:273 */
#define QH_ERR_H3_FRAME_ERROR (-602)             /* nghttp3.h:280 */
#define QH_ERR_H3_GENERAL_PROTOCOL_ERROR (-606)  /* nghttp3.h:307 */

#define QH_H3_OPEN 0 /* status: the stream goes on                         */
#define QH_H3_END 1  /* status: the message ended (MSG_END)                */
#define QH_H3_WAIT 2 /* status: settle first, then feed from consumed on   */

#define QH_H3_ST_FRAME_TYPE 0
#define QH_H3_ST_FRAME_LENGTH 1
#define QH_H3_ST_DATA 2
#define QH_H3_ST_HEADERS 3
#define QH_H3_ST_IGN_FRAME 4
#define QH_H3_ST_IGN_REST 5

#define QH_H3_F_NONE 0
#define QH_H3_F_DATA 1    /* NGHTTP3_FRAME_DATA 0x00, lib/nghttp3_frame.h:37 */
#define QH_H3_F_HEADERS 2 /* NGHTTP3_FRAME_HEADERS 0x01                      */
#define QH_H3_F_REFUSED 3 /* the eleven types of conn.c:1643-1653            */
#define QH_H3_F_UNKNOWN 4

#define QH_H3_RESPONSE 0x1u
#define QH_H3_PENDING 0x2u  /* a HEADERS section is on its way through the check */
#define QH_H3_SAW_DATA 0x4u /* ... and a DATA frame began behind it              */
#define QH_H3_SAW_END 0x8u  /* ... and the stream ended behind it                */

typedef struct qh_h3_stream { /* 32 B */
  uint64_t left;
  uint64_t acc;
  int64_t recv;
  uint8_t state, vleft, fclass, hstate;
  uint16_t flags;
  int16_t err;
} qh_h3_stream;
/* FRAME_TYPE, REQ_INITIAL (response != 0: RESP_INITIAL and QH_H3_RESPONSE). */
QH_EXPORT void qh_h3_stream_init(qh_h3_stream *rs, size_t n, int response);

QH_EXPORT int qh_qpack_h3_read(
    const uint8_t *src, const qh_span_in *chunks, const uint8_t *chunk_fin,
    const uint64_t *chunk_sid, const uint32_t *chunk_view, size_t nchunks, qh_h3_stream *rs,
    const qh_http_state *hs, int32_t *status, uint32_t *consumed, uint32_t *nunknown,
    qh_span_in *pieces, uint64_t *piece_sid, uint32_t *piece_view, uint8_t *piece_fin,
    uint8_t *piece_kind, uint64_t *npieces, uint64_t *dspan_start, qh_span_in *dspans,
    uint64_t dspan_cap, uint64_t *ndspans);
QH_EXPORT int qh_h3_read_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *chunks, const uint8_t *chunk_fin,
    const uint64_t *chunk_sid, const uint32_t *chunk_view, size_t nchunks, qh_h3_stream *rs,
    const qh_http_state *hs, int32_t *status, uint32_t *consumed, uint32_t *nunknown,
    qh_span_in *pieces, uint64_t *piece_sid, uint32_t *piece_view, uint8_t *piece_fin,
    uint8_t *piece_kind, uint64_t *npieces, uint64_t *dspan_start, qh_span_in *dspans,
    uint64_t dspan_cap, uint64_t *ndspans, int where);

QH_EXPORT int qh_qpack_h3_settle(qh_h3_stream *rs, const qh_http_state *hs,
                                 const int32_t *sec_status, size_t n, int32_t *status);
QH_EXPORT int qh_h3_settle_batch(qh_ctx *ctx, qh_h3_stream *rs, const qh_http_state *hs,
                                 const int32_t *sec_status, size_t n, int32_t *status, int where);

/* ---- Response and request streams as they leave: HTTP/3 frames written ------
 *
 * What nghttp3_stream_write_header_block and nghttp3_stream_write_data put in
 * front of a field section and of body bytes (lib/nghttp3_stream.c:492-703:
 * nghttp3_frame_write_hd, lib/nghttp3_frame.c:34-43, two shortest-form varints
 * as nghttp3_put_uvarint writes them), for many streams in one call.  The
 * sections lie where qh_encode_fields_batch, qh_encode_fields_dyn_batch or
 * qh_encode_conns_batch left them (dst and sections[]), the bodies in a second
 * buffer; the call writes the bytes of each stream's frames, contiguous and in
 * stream order, into one buffer.  A host form over host pointers and a device
 * form over pointers in HBM (where must be QH_WHERE_DEVICE; counts are host
 * scalars); both compile the same rules (csrc/qh_h3w_core.h) and agree byte
 * for byte on every output and every record.
 *
 * qh_h3_item is one frame to write (32 B):
 *   span   the payload, bytes [off, off + len) of one of the two sources
 *          (span.flags is ignored);
 *   type   the frame type: 0 DATA, 1 HEADERS (lib/nghttp3_frame.h:37-38); any
 *          other value up to 2^62 - 1 is written as given, so a caller can send
 *          a frame whose payload it built itself, or a reserved type;
 *   src    0: hsrc (the section writer's dst, so that sections[k] goes in as it
 *          is), 1: dsrc (bodies);
 *   flags  QH_H3W_END: the stream ends after this item.  This is the
 *          reference's NGHTTP3_STREAM_FLAG_WRITE_END_STREAM: a request or
 *          response submitted without a data reader (conn.c:2553-2555, :2591-2593), a data
 *          reader's EOF without NGHTTP3_DATA_FLAG_NO_END_STREAM
 *          (stream.c:641-644), or trailers (conn.c:2614).
 * qh_h3_tx is the per-stream record, caller-owned, beside the stream's other
 * records (16 B): off, the stream offset of the next byte, which is the sum of
 * everything written so far; flags, QH_H3W_ENDED; rsv, zero.
 *
 * write.  Stream s owns items[item_start[s], item_start[s + 1]) (item_start has
 * nstreams + 1 entries) and tx[s].  Per stream:
 *   out[s]     a span into dst: the bytes of stream s of this call, contiguous,
 *              the streams in order (out[s].off is the sum of the lengths
 *              before it);
 *   fin[s]     1 when this call ended the stream;
 *   status[s]  0 or QH_ERR_INVALID_STATE.
 * out, fin, a stream-id array and a view array are exactly the chunks,
 * chunk_fin, chunk_sid and chunk_view of qh_h3_read_batch on the peer, with
 * dst as its src.  Rules per stream, items in order:
 *   1. (the project's own rule) tx[s].flags has QH_H3W_ENDED and the stream has
 *      at least one item, or an item follows one that carries QH_H3W_END in
 *      the same call: status QH_ERR_INVALID_STATE, nothing is written for the
 *      stream, out[s].len and fin[s] are 0, the record is unchanged, and the
 *      other streams proceed.  The reference answers this only for trailers
 *      (conn.c:2610-2612) and leaves the other submits as a TODO
 *      (conn.c:2564, :2582, :2602);
 *   2. a DATA item of length 0 writes no frame (stream.c:645-663); its
 *      QH_H3W_END still ends the stream;
 *   3. every other item writes qh_h3_write_hd(type, len) followed by the len
 *      payload bytes (stream.c:666-700; HEADERS :521-535).  A HEADERS item of
 *      length 0 is written as it is.  Payloads and the order of frames are not
 *      judged; the reference does not judge them either;
 *   4. fin[s] is 1 and the record gains QH_H3W_ENDED iff an item carried
 *      QH_H3W_END; tx[s].off advances by out[s].len.  A stream without items
 *      has length 0, fin 0, status 0.
 * Returns 0; QH_ERR_INVALID_ARGUMENT with nothing written for a NULL argument
 * that is needed (dst_need; with streams item_start, tx, out, fin, status;
 * items when a stream has one; the source of an item that has bytes; dst when
 * bytes are to be written and dst_cap has room), nstreams of 2^27 or more,
 * an item_start that decreases, a type of 2^62 or more, src above 1, an item
 * flag or a record flag that is not defined (or rsv not 0), or a stream whose
 * bytes of this call pass 2^32 - 1; QH_ERR_NOMEM when dst_cap is short, with
 * the exact need in *dst_need and nothing else written (no dst, out, fin,
 * status or record; a NULL dst with dst_cap 0 is the sizing call).  *dst_need
 * is the sum of the out lengths after every other return of 0.  No byte
 * outside an item's span is read and no byte outside [dst, dst + need) is
 * written: the sources and dst need neither padding nor alignment.
 *
 * Device: a lane per stream checks and counts (qh_k_h3w_count), one scan over
 * two segments, one host wait (the byte total, the long payloads' pieces, the
 * list's errors), then a 16-lane group per stream places its frames, writes
 * the headers and copies the payloads below QH_OPT_H3W_LONG_MIN bytes
 * (qh_k_h3w_write); longer payloads are listed in pieces of at most
 * QH_OPT_H3W_PIECE bytes and copied a wave per piece (qh_k_emit_copy_long).
 *
 * qh_h3_write_hd / qh_h3_write_hd_len are host drop-ins for
 * nghttp3_frame_write_hd / nghttp3_frame_write_hd_len (frame.c:34-43): type
 * and len below 2^62, p with room for qh_h3_write_hd_len bytes (at most 16);
 * the return is the byte behind the header.
 *
 * Departures: the output is one contiguous run per stream, copied (the
 * reference hands writev_stream a vector list and never copies a body); one
 * DATA item is one frame (the reference joins up to eight vectors of one
 * read_data call, stream.c:613-634); flow control, add_write_offset and the
 * retention of unacknowledged bytes stay with the caller's QUIC stream
 * buffer, of which dst is the input, as the reader leaves the unread tail
 * there.  Not built: the GOAWAY / PRIORITY_UPDATE payloads (a caller sends
 * them as an item with its own payload; the control stream's opening bytes
 * are qh_h3_write_settings), a vector-list output without the copy,
 * QH_WHERE_HOST staging. */
#define QH_ERR_INVALID_STATE (-102) /* nghttp3.h:175 */

#define QH_H3W_END 0x1u   /* qh_h3_item.flags: the stream ends after this item */
#define QH_H3W_ENDED 0x1u /* qh_h3_tx.flags: the stream has ended              */

typedef struct qh_h3_item { /* 32 B */
  qh_span_in span;
  uint64_t type;
  uint32_t src;
  uint32_t flags;
} qh_h3_item;

typedef struct qh_h3_tx { /* 16 B */
  uint64_t off;
  uint32_t flags;
  uint32_t rsv;
} qh_h3_tx;
/* off 0, no flags. */
QH_EXPORT void qh_h3_tx_init(qh_h3_tx *tx, size_t n);

QH_EXPORT uint8_t *qh_h3_write_hd(uint8_t *p, uint64_t type, uint64_t len);
QH_EXPORT size_t qh_h3_write_hd_len(uint64_t type, uint64_t len);

QH_EXPORT int qh_qpack_h3_write(
    const uint8_t *hsrc, const uint8_t *dsrc, const qh_h3_item *items, const uint32_t *item_start,
    size_t nstreams, qh_h3_tx *tx, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_need,
    qh_span_in *out, uint8_t *fin, int32_t *status);
QH_EXPORT int qh_h3_write_batch(
    qh_ctx *ctx, const uint8_t *hsrc, const uint8_t *dsrc, const qh_h3_item *items,
    const uint32_t *item_start, size_t nstreams, qh_h3_tx *tx, uint8_t *dst, uint64_t dst_cap,
    uint64_t *dst_need, qh_span_in *out, uint8_t *fin, int32_t *status, int where);

/* ---- Unidirectional streams as they arrive: types, control frames, SETTINGS --
 *
 * What nghttp3_conn_read_uni does with the bytes of the peer's unidirectional
 * streams (lib/nghttp3_conn.c:631-721): the stream type varint
 * (conn_read_type, :570-625), which stream may open and which may not open
 * twice, the control stream's frames (nghttp3_conn_read_control, :732-1340:
 * SETTINGS first and once, GOAWAY, MAX_PUSH_ID, PRIORITY_UPDATE, the refused
 * and the ignored types) and the peer's SETTINGS put to this side's QPACK
 * encoder (nghttp3_conn_on_settings_entry_received, :1960-2052), for the
 * chunks of many connections in one call.  The bytes behind the type of the
 * QPACK encoder and decoder streams come out as spans that go as they are
 * into qh_ustream_join_batch.  Each call has a host form over host pointers
 * and a device form over pointers in HBM (where must be QH_WHERE_DEVICE;
 * counts are host scalars); both compile the same rules (csrc/qh_h3u_core.h)
 * and agree byte for byte on every output and every record.
 *
 * qh_h3_uni is the per-stream record, caller-owned (32 B):
 *   left    rstate->left: payload bytes of the frame in progress still to come;
 *   acc     rvint->acc: the value of the bytes of a cut varint read so far;
 *   aux     the SETTINGS identifier whose value is still to come, or the
 *           PRIORITY_UPDATE element id;
 *   state   QH_H3U_ST_* (NGHTTP3_CTRL_STREAM_STATE_*, lib/nghttp3_stream.h:62-75);
 *   vleft   rvint->left: the bytes of the cut varint still missing (0 to 7);
 *   type    QH_H3U_T_NONE (not identified yet), _CONTROL, _QENC, _QDEC, _UNKNOWN;
 *   ftype   QH_H3U_F_*: the class of the frame in progress;
 *   flags   zero;
 *   err     the first error, latched (0: none).
 * qh_h3_conn is the per-connection record, caller-owned (64 B): the remote
 * settings (max_field_section_size, 2^62 - 1 until the peer says otherwise,
 * conn.c:357; qpack_max_dtable_capacity; qpack_blocked_streams;
 * QH_H3C_CONNECT_PROTOCOL and QH_H3C_H3_DATAGRAM in flags), goaway_id (2^62
 * until a GOAWAY arrives, conn.c:361), max_pushes, max_client_streams (the
 * caller's: the bound of the PRIORITY_UPDATE id check, conn.c:2061-2064),
 * pri_buf / pri_len (rx.pri_fieldbuf, lib/nghttp3_conn.h:137: a Priority Field
 * Value that arrives in parts), flags (the reference's NGHTTP3_CONN_FLAG_*
 * values for SETTINGS_RECVED, CONTROL_OPENED, QPACK_ENCODER_OPENED,
 * QPACK_DECODER_OPENED and GOAWAY_RECVED; QH_H3C_SERVER; the two setting
 * booleans; QH_H3C_CAP_NEW and QH_H3C_BLOCKED_NEW, see apply) and err, the
 * connection's first error, latched: every error here is a connection error
 * in the reference.
 * qh_h3_event is what the callbacks would have delivered (32 B): kind
 * (QH_H3_EV_SETTINGS: recv_settings, the values are in the connection record;
 * QH_H3_EV_GOAWAY: shutdown, id the GOAWAY id; QH_H3_EV_PRIORITY_UPDATE: id
 * the element id, value[0, len) the Priority Field Value, len 0 the empty
 * update of conn.c:1116-1127; QH_H3_EV_STOP_SENDING: an unknown stream type
 * identified without fin, conn.c:676-682, id the stream id), chunk (the chunk
 * that produced it), id, value[8] (zero behind len), len.
 *
 * read.  Chunk c is src[chunks[c].off, + len), the new bytes of stream
 * chunk_sid[c], chunk_fin[c] != 0 when they end it, with its record us[c] (the
 * caller gathers and scatters).  Connection k owns cs[k] and the chunks
 * [conn_start[k], conn_start[k + 1]) in arrival order (conn_start has nconns +
 * 1 entries, begins at 0, does not decrease and ends at nchunks: the
 * convention of qh_encode_conns_batch).  A stream appears at most once per
 * call.  Per chunk: status[c] (QH_H3U_OPEN, QH_H3U_GONE: the stream was closed
 * before any byte of its type and the reference deletes it, conn.c:641-657; or
 * the error) and consumed[c].  Per connection: nglitch[k] (optional), the
 * times the reference would have drained its rate limiter (a zero-length
 * closed stream, an unknown stream type, PRIORITY_UPDATE, ORIGIN, an unknown
 * frame, a GOAWAY or MAX_PUSH_ID that repeats the current value); the limiter
 * is timed, so its verdict (-610) is the caller's.  Compacted in chunk order:
 * enc_pieces[j] / enc_conn[j], *nenc: the bytes behind the type of QPACK
 * encoder streams as spans into src with their connection index (pieces / tsel
 * / nsel of qh_ustream_join_batch on the table side); dec_pieces / dec_conn,
 * *ndec: the same for the decoder stream (qh_enc_read_decoder_batch's side).
 * Room for nchunks entries in each always suffices and is required.  events,
 * *nevents: when event_cap is short the call returns QH_ERR_NOMEM with the
 * exact need in *nevents and nothing else written.  Rules per connection, its
 * chunks in order, in the reference's order:
 *   1. an error is latched in the connection (or the stream) record: status
 *      is that error, consumed 0, nothing changes;
 *   2. while the record's type is QH_H3U_T_NONE the stream id must be a
 *      unidirectional stream of the peer (low two bits 2 for a server reading,
 *      3 for a client), else -609 (conn.c:513-545); an empty chunk without fin
 *      changes nothing;
 *   3. the type (conn.c:640-688).  An empty chunk with fin is -606 when a
 *      varint is cut, else QH_H3U_GONE and one glitch.  The varint is
 *      continued from the record; one cut by fin is -606.  0 is the control
 *      stream, 2 the QPACK encoder stream, 3 the QPACK decoder stream: each
 *      sets its flag or is -609 when the flag is set already; 1 (push) is
 *      -609; any other type is unknown: one glitch, a STOP_SENDING event
 *      unless fin, and this and every later chunk of the stream is consumed
 *      whole.  With nothing left behind the type the chunk ends here, before
 *      the fin test (conn.c:685-687);
 *   4. an identified stream with bytes or fin: fin on a control, encoder or
 *      decoder stream is -605; encoder and decoder streams yield their piece
 *      (none of their bytes is read); the control stream is walked as
 *      read_control walks it: cut varints continued from the record; a first
 *      frame other than SETTINGS is -603, a second SETTINGS -601; inside
 *      SETTINGS a varint that crosses the frame's end and an identifier with
 *      no value are -602, and every entry is judged as it completes (a second
 *      nonzero table capacity or blocked-streams value -608, the four HTTP/2
 *      identifiers -608, ENABLE_CONNECT_PROTOCOL ignored by a server and 0 or
 *      1 on a client, never back to 0, H3_DATAGRAM 0 or 1, unknown identifiers
 *      ignored); an empty SETTINGS frame is delivered too; GOAWAY of length 0
 *      is -602, on a client an id that is no client bidirectional stream -607,
 *      an increase -607, a repeat one glitch; MAX_PUSH_ID on a client -601,
 *      length 0 -602, a decrease -602, a repeat one glitch (after the varint
 *      of either the stream is back in the type state whatever the length
 *      said, conn.c:1064, :1095); PRIORITY_UPDATE (0xF0700) on a client -601,
 *      length 0 -602, one glitch, the element id checked when the frame ends
 *      (-607), a value of more than 8 bytes turns the rest of the frame into
 *      an ignored one; 0xF0701 is -607; ORIGIN (taken as the reference takes
 *      it with no origin callbacks set) and every unknown type are one glitch
 *      and skipped; the eight types of conn.c:875-883 are -601;
 *   5. a chunk that ends in an error leaves no trace but the error: no piece,
 *      no events and no glitches of that chunk, both records as on entry to
 *      the chunk with the error latched in each, consumed 0.
 * Returns 0; QH_ERR_INVALID_ARGUMENT with nothing written for a NULL argument
 * that is needed, a bad conn_start, nchunks of 2^27 or more, or a stream or
 * connection record that no call here leaves; QH_ERR_NOMEM as above.  No byte
 * outside a chunk is read: src needs no padding.  Device: a lane per
 * connection walks its chunks on copies of the records and counts
 * (qh_k_h3u_count), one scan over three segments, one host wait (the three
 * totals and the list's errors), then a lane per connection replays the walk
 * and writes (qh_k_h3u_write).  The lane is per connection because which
 * stream may open and whether SETTINGS has been seen is connection state that
 * the chunks of one call change in order.
 *
 * apply.  For each listed connection (csel[j] < nconns; NULL: all nconns,
 * whatever nsel says) whose record has QH_H3C_CAP_NEW: what
 * qh_enc_state_set_capacity(&enc[k], &acct[k], qpack_max_dtable_capacity)
 * does; with QH_H3C_BLOCKED_NEW: enc[k].max_blocked = min(100,
 * qpack_blocked_streams) (conn.c:2007-2008).  Both bits are cleared.  The read
 * sets them when the nonzero entry is received, which is when the reference
 * calls its encoder.  A csel entry of nconns or more, or a connection named
 * twice: host QH_ERR_INVALID_ARGUMENT with nothing written, device passed over
 * (as qh_ustream_sections_batch does).  The device form is a lane per listed
 * connection, asynchronous on the context stream, with no host wait.
 *
 * qh_h3_write_settings writes the opening bytes of this side's control stream
 * as nghttp3_stream_write_stream_type and nghttp3_stream_write_settings do
 * (lib/nghttp3_stream.c:309-390): the type 0x00, then a SETTINGS frame with
 * the identifiers 0x06, 0x01, 0x07 in that order, always, then 0x33 = 1 and
 * 0x08 = 1 when set, every varint in its shortest form.  Values below 2^62;
 * dst NULL: only the length (at most 64) is returned.  Host only.  GOAWAY and
 * PRIORITY_UPDATE need no call: qh_h3_write_batch writes any frame type around
 * a payload the caller built.
 *
 * Departures: the Priority Field Value is handed out, not parsed (the
 * reference's parser for it is not part of this library, and `priority` is
 * left unparsed for the same reason), so the -606 of conn.c:1182-1186 is the
 * caller's; finding the prioritised stream (conn.c:2066) is qh_h3_find_batch's,
 * creating it (:2074-2097) stays with the caller; ORIGIN is not delivered; the
 * rate limiter's verdict is the caller's; a stream closed before any byte is
 * counted as a glitch whether or not an empty chunk came before (the record
 * does not tell).  Not built: QH_WHERE_HOST staging. */
#define QH_ERR_H3_MISSING_SETTINGS (-603)        /* nghttp3.h:287 */
#define QH_ERR_H3_CLOSED_CRITICAL_STREAM (-605)  /* nghttp3.h:300 */
#define QH_ERR_H3_ID_ERROR (-607)                /* nghttp3.h:314 */
#define QH_ERR_H3_SETTINGS_ERROR (-608)          /* nghttp3.h:321 */
#define QH_ERR_H3_STREAM_CREATION_ERROR (-609)   /* nghttp3.h:329 */

#define QH_H3U_OPEN 0 /* status: the stream goes on              */
#define QH_H3U_GONE 1 /* status: closed before a byte of its type */

#define QH_H3U_ST_FRAME_TYPE 0
#define QH_H3U_ST_FRAME_LENGTH 1
#define QH_H3U_ST_SETTINGS 2
#define QH_H3U_ST_GOAWAY 3
#define QH_H3U_ST_MAX_PUSH_ID 4
#define QH_H3U_ST_IGN_FRAME 5
#define QH_H3U_ST_SETTINGS_ID 6
#define QH_H3U_ST_SETTINGS_VALUE 7
#define QH_H3U_ST_PRIORITY_UPDATE_PRI_ELEM_ID 8
#define QH_H3U_ST_PRIORITY_UPDATE 9

#define QH_H3U_T_NONE 0
#define QH_H3U_T_CONTROL 1
#define QH_H3U_T_QENC 2
#define QH_H3U_T_QDEC 3
#define QH_H3U_T_UNKNOWN 4

#define QH_H3U_F_NONE 0
#define QH_H3U_F_SETTINGS 1             /* 0x04 */
#define QH_H3U_F_GOAWAY 2               /* 0x07 */
#define QH_H3U_F_MAX_PUSH_ID 3          /* 0x0d */
#define QH_H3U_F_PRIORITY_UPDATE 4      /* 0xf0700 */
#define QH_H3U_F_PRIORITY_UPDATE_PUSH 5 /* 0xf0701 */
#define QH_H3U_F_ORIGIN 6               /* 0x0c */
#define QH_H3U_F_REFUSED 7              /* the eight types of conn.c:875-883 */
#define QH_H3U_F_UNKNOWN 8

#define QH_H3C_SETTINGS_RECVED 0x0001u /* NGHTTP3_CONN_FLAG_*, lib/nghttp3_conn.h:54-69 */
#define QH_H3C_CONTROL_OPENED 0x0002u
#define QH_H3C_QENC_OPENED 0x0004u
#define QH_H3C_QDEC_OPENED 0x0008u
#define QH_H3C_GOAWAY_RECVED 0x0020u
#define QH_H3C_SERVER 0x0100u
#define QH_H3C_CONNECT_PROTOCOL 0x0200u /* remote enable_connect_protocol */
#define QH_H3C_H3_DATAGRAM 0x0400u      /* remote h3_datagram             */
#define QH_H3C_CAP_NEW 0x0800u          /* a table capacity to apply      */
#define QH_H3C_BLOCKED_NEW 0x1000u      /* a blocked-streams value to apply */

#define QH_H3_EV_SETTINGS 1
#define QH_H3_EV_GOAWAY 2
#define QH_H3_EV_PRIORITY_UPDATE 3
#define QH_H3_EV_STOP_SENDING 4

typedef struct qh_h3_uni { /* 32 B */
  uint64_t left;
  uint64_t acc;
  uint64_t aux;
  uint8_t state, vleft, type, ftype;
  uint16_t flags;
  int16_t err;
} qh_h3_uni;

typedef struct qh_h3_conn { /* 64 B */
  uint64_t max_field_section_size;
  uint64_t qpack_max_dtable_capacity;
  uint64_t qpack_blocked_streams;
  uint64_t goaway_id;
  uint64_t max_pushes;
  uint64_t max_client_streams;
  uint8_t pri_buf[8];
  uint8_t pri_len, rsv;
  uint16_t flags;
  int16_t err;
  uint16_t rsv2;
} qh_h3_conn;

typedef struct qh_h3_event { /* 32 B */
  uint32_t kind;
  uint32_t chunk;
  uint64_t id;
  uint8_t value[8];
  uint32_t len;
  uint32_t rsv;
} qh_h3_event;

/* Not identified, the type state, no error. */
QH_EXPORT void qh_h3_uni_init(qh_h3_uni *us, size_t n);
/* The reference's conn_new values; server != 0: QH_H3C_SERVER. */
QH_EXPORT void qh_h3_conn_init(qh_h3_conn *cs, size_t n, int server, uint64_t max_client_streams);

QH_EXPORT int qh_qpack_h3_uni_read(
    const uint8_t *src, const qh_span_in *chunks, const uint8_t *chunk_fin,
    const uint64_t *chunk_sid, size_t nchunks, const uint32_t *conn_start, size_t nconns,
    qh_h3_uni *us, qh_h3_conn *cs, int32_t *status, uint32_t *consumed, uint32_t *nglitch,
    qh_span_in *enc_pieces, uint32_t *enc_conn, uint64_t *nenc, qh_span_in *dec_pieces,
    uint32_t *dec_conn, uint64_t *ndec, qh_h3_event *events, uint64_t event_cap,
    uint64_t *nevents);
QH_EXPORT int qh_h3_uni_read_batch(
    qh_ctx *ctx, const uint8_t *src, const qh_span_in *chunks, const uint8_t *chunk_fin,
    const uint64_t *chunk_sid, size_t nchunks, const uint32_t *conn_start, size_t nconns,
    qh_h3_uni *us, qh_h3_conn *cs, int32_t *status, uint32_t *consumed, uint32_t *nglitch,
    qh_span_in *enc_pieces, uint32_t *enc_conn, uint64_t *nenc, qh_span_in *dec_pieces,
    uint32_t *dec_conn, uint64_t *ndec, qh_h3_event *events, uint64_t event_cap,
    uint64_t *nevents, int where);

QH_EXPORT int qh_qpack_h3_settings_apply(qh_h3_conn *cs, const uint32_t *csel, size_t nsel,
                                         size_t nconns, qh_dtable_acct *acct, qh_enc_state *enc);
QH_EXPORT int qh_h3_settings_apply_batch(qh_ctx *ctx, qh_h3_conn *cs, const uint32_t *csel,
                                         size_t nsel, size_t nconns, qh_dtable_acct *acct,
                                         qh_enc_state *enc, int where);

typedef struct qh_h3_settings { /* what qh_h3_write_settings announces */
  uint64_t max_field_section_size;
  uint64_t qpack_max_dtable_capacity;
  uint64_t qpack_blocked_streams;
  uint8_t enable_connect_protocol, h3_datagram;
  uint8_t rsv[6];
} qh_h3_settings;
QH_EXPORT size_t qh_h3_write_settings(uint8_t *dst, const qh_h3_settings *s);

/* ---- Streams by id: a per-connection stream table, arrivals routed ----------
 *
 * The top of the reference's receive path, which the calls above leave to
 * their caller: finding a stream by its id, creating it when the id is new,
 * refusing ids that may not open (nghttp3_conn_read_stream2,
 * lib/nghttp3_conn.c:468-568; nghttp3_conn_create_stream / _find_stream,
 * :2135-2171; conn_bidi_idtr_open, :446-459, lib/nghttp3_idtr.c,
 * lib/nghttp3_gaptr.c), closing it (nghttp3_conn_close_stream2 :2772-2790,
 * conn_delete_stream :1342-1403), the GOAWAY id (nghttp3_conn_shutdown,
 * _submit_shutdown_notice, :2619-2669) and the create half of
 * nghttp3_conn_submit_request (:2538-2549), for many connections in one call.
 * Each call has a host form over host pointers and a device form over pointers
 * in HBM (where must be QH_WHERE_DEVICE; counts are host scalars); both
 * compile the same rules (csrc/qh_h3d_core.h) and agree byte for byte on every
 * output, every record and every slot, entry and gap.
 *
 * State, caller-owned, named by one qh_h3d_tab (a host structure of pointers):
 *   sm[nconns]     qh_h3_smap, one per connection (64 B): its regions
 *                  (slot_off, nslots, rec_off, rec_cap, gap_off, in units of
 *                  slots, records and gaps), nlive, the free-list head
 *                  (free_head: local record index + 1, 0: none) and high-water
 *                  mark (hiwater) of its records, num_streams
 *                  (remote.bidi.num_streams: a server's live client bidi
 *                  streams), max_stream_id_bidi (-4 at first, conn.c:363),
 *                  tx_goaway_id (2^62 at first, conn.c:362), ngaps, call (the
 *                  number of the last dispatch call, which a routed entry
 *                  remembers), flags (QH_H3M_*) and err, the first error of a
 *                  dispatch, latched;
 *   slots[nslots]  uint32_t: 0, or local record index + 1.  The home slot of
 *                  stream id x in a region of n slots (n a power of two, at
 *                  least 2 and at least 2 rec_cap) is
 *                    ((uint32_t)((x * 0x9E3779B97F4A7C15) >> 32)) & (n - 1)
 *                  (the product modulo 2^64); a stream lies at the first free
 *                  slot from there on, cyclically, and a removal shifts the
 *                  run behind it back (no tombstones), so the slot bytes
 *                  depend only on the order of inserts and removals;
 *   ents[nrecs]    qh_h3_sent, one per record (32 B): stream_id, the raw
 *                  Priority Field Value (pri_buf, pri_len, as qh_h3_event
 *                  carries it), next (the free-list link), call, flags
 *                  (QH_H3S_LIVE and the reference's NGHTTP3_STREAM_FLAG_*
 *                  values READ_EOF, SHUT_RD, SERVER_PRIORITY_SET,
 *                  PRIORITY_UPDATE_RECVED).  A record's index, rec_off + local
 *                  index, is stable for the stream's life, reused after a
 *                  close (last freed, first reused; else the high-water mark)
 *                  and indexes rs_pool, hs_pool, us_pool and any pool the
 *                  caller keeps beside them (qh_h3_tx);
 *   gaps[ngaps]    qh_h3_gap (begin, end), 33 per connection: the
 *                  nghttp3_gaptr of remote.bidi.idtr as a sorted array over
 *                  stream_id >> 2; none: nothing pushed yet.  A list longer
 *                  than 32 after an open drops its first gap (conn.c:454-456);
 *   rs_pool, hs_pool, us_pool  nrecs records each.
 * qh_h3_smap_init lays the regions of n connections out back to back in
 * connection order (nslots the least power of two >= max(2, 2 rec_cap[k])),
 * sets the reference's initial values and returns the three totals (slots,
 * records, gaps); slots, ents and gaps start zeroed.  rec_cap[k] is the
 * caller's bound on live streams (the QUIC stream limits plus the peer's
 * unidirectional streams).
 *
 * dispatch.  Connection k owns arrivals [conn_start[k], conn_start[k + 1]) in
 * arrival order (the convention of qh_h3_uni_read_batch); arrival a is
 * stream_id[a], chunks[a] (a span the call only hands on) and fin[a].  Per
 * arrival route[a] and rec[a] (the record index, UINT32_MAX: none), in the
 * reference's order:
 *   1. an error latched in the connection: route is that error;
 *   2. the stream is found and was routed earlier in this call: QH_H3D_AGAIN,
 *      nothing changes (the calls below take a stream once per call; the
 *      caller feeds the arrival in its next call);
 *   3. not found.  Server: a client bidi id (low bits 0) opens its id in the
 *      gap list (an in-use answer is ignored, conn.c:490-494), raises
 *      max_stream_id_bidi and num_streams and is created; behind a queued
 *      GOAWAY with tx_goaway_id <= id its record starts in QH_H3_ST_IGN_REST
 *      and the route of this arrival is QH_H3D_BIDI_REJECTED (the caller
 *      sends STOP_SENDING and RESET_STREAM with 0x010B: conn_reject_stream);
 *      a client uni id (2) with no bytes and fin creates nothing
 *      (QH_H3D_NONE), else is created; ids 1 and 3 are -609.  Client: a
 *      server uni id (3) likewise; ids 0, 1, 2 are -609.  A table with
 *      rec_cap live streams is -901 (nghttp3_map_insert's failure; the limit
 *      is this library's, tested before anything changes).  A created stream's
 *      pool records are as qh_h3_stream_init (REQ_INITIAL on a server,
 *      RESP_INITIAL and QH_H3_RESPONSE on a client), qh_http_state_init and
 *      qh_h3_uni_init leave them;
 *   4. no bytes and no fin: QH_H3D_NONE (the stream stays created; a rejected
 *      creation is QH_H3D_BIDI_REJECTED all the same), and it joins no list;
 *   5. fin sets QH_H3S_READ_EOF; the route is QH_H3D_UNI for ids 2 and 3, else
 *      QH_H3D_BIDI (or _REJECTED, rule 3), and the arrival joins its list.
 * A negative route is latched in sm[k].err.  The lists, compacted in arrival
 * order, with room for narrivals entries each (required, so there is no NOMEM
 * case): b_chunks, b_fin, b_sid, b_view (= k), b_rec and the gathered rs_call,
 * hs_call go as they are into qh_h3_read_batch; u_chunks, u_fin, u_sid, u_rec,
 * u_conn_start (nconns + 1 entries) and us_call into qh_h3_uni_read_batch.
 * Returns 0; QH_ERR_INVALID_ARGUMENT with nothing written for a needed NULL, a
 * bad conn_start, or a connection record, region or slot that no call here
 * leaves (nslots no power of two, a region outside its array, a slot naming a
 * record that is not live, nlive not the number of used slots).  Regions of
 * two connections must not overlap (qh_h3_smap_init's layout; not checked).
 *
 * commit scatters rs_call / hs_call by b_rec and us_call by u_rec back into
 * the pools after the round's last call.  An index out of range or named twice
 * is passed over and counted in *nskipped (host: the first in list order is
 * kept; device: a word in HBM, one of the two is kept).
 *
 * open: the create half of submit_request for items [conn_start[k],
 * conn_start[k + 1]) of a client connection k, in order: the connection's
 * latched error; -101 on a server or for an id that is no client bidi id; -111
 * after QH_H3C_GOAWAY_RECVED in cs[k]; -104 when found; -901 when full; else
 * created with RESP_INITIAL records, rec[j] its index.
 *
 * find writes rec[j] for (conn[j], stream_id[j]), or UINT32_MAX.
 * recs_move gathers (dir 0: call[j] = pool[idx[j]]) or scatters (dir 1) records
 * of 16, 32 or 64 bytes; an idx of npool or more is passed over.  Both arrays
 * 16-byte aligned on the device.
 *
 * close: close_stream2 for items grouped by conn_start, in order: -110 when
 * not found; -605 for a uni stream whose us_pool type is QH_H3U_T_CONTROL,
 * _QENC or _QDEC (QH_H3U_T_NONE and QH_H3U_T_UNKNOWN are the reference's
 * NGHTTP3_STREAM_TYPE_UNKNOWN, which may close); else the entry leaves the
 * table, its record goes to the free list, num_streams falls for a server's
 * client bidi stream.  cancel_sid / cancel_view, *ncancel: every closed bidi
 * stream, compacted in list order, for qh_dec_blocked_cancel_batch and
 * qh_dec_partial_cancel_batch (the reference cancels a blocked stream only;
 * both calls answer removed = 0 for a stream they do not hold).  drained[k]:
 * QH_H3M_SHUTDOWN_COMMENCED and num_streams == 0 (conn.c:3023-3024; the
 * control stream's queue is the caller's).
 *
 * shutdown, per listed connection (csel as in apply above): kind
 * QH_H3D_NOTICE sets tx_goaway_id to 2^62 - 4 (client: 2^62 - 1) and
 * QH_H3M_GOAWAY_QUEUED; QH_H3D_SHUTDOWN to min(2^62 - 4, max_stream_id_bidi +
 * 4) (client: 0) and QH_H3M_SHUTDOWN_COMMENCED too.  goaway_id[j] is the id to
 * frame with qh_h3_write_batch.  An id above the current one (the reference's
 * assert) is status -101 with nothing changed.
 *
 * Departures: the reference's robin-hood nghttp3_map is not observable and is
 * not copied; a stream twice in one call is answered QH_H3D_AGAIN; -901 comes
 * from rec_cap.  Not built: priority_resolve (conn_on_priority_update_stream,
 * conn.c:2054-2107, for the events of a uni read), QH_WHERE_HOST staging. */
#define QH_ERR_STREAM_IN_USE (-104)    /* nghttp3.h:189 */
#define QH_ERR_STREAM_NOT_FOUND (-110) /* nghttp3.h:231 */
#define QH_ERR_CONN_CLOSING (-111)     /* nghttp3.h:238 */

#define QH_H3D_NONE 0
#define QH_H3D_BIDI 1
#define QH_H3D_BIDI_REJECTED 2
#define QH_H3D_UNI 3
#define QH_H3D_AGAIN 4

#define QH_H3D_NOTICE 0
#define QH_H3D_SHUTDOWN 1

#define QH_H3D_GAPS 33 /* gaps per connection */

#define QH_H3M_SERVER 0x01u
#define QH_H3M_GOAWAY_QUEUED 0x40u      /* NGHTTP3_CONN_FLAG_GOAWAY_QUEUED      */
#define QH_H3M_SHUTDOWN_COMMENCED 0x80u /* NGHTTP3_CONN_FLAG_SHUTDOWN_COMMENCED */

#define QH_H3S_LIVE 0x0001u
#define QH_H3S_READ_EOF 0x0020u /* NGHTTP3_STREAM_FLAG_*, lib/nghttp3_stream.h:116-131 */
#define QH_H3S_SHUT_RD 0x0200u
#define QH_H3S_SERVER_PRIORITY_SET 0x0400u
#define QH_H3S_PRIORITY_UPDATE_RECVED 0x0800u

typedef struct qh_h3_smap { /* 64 B */
  uint32_t slot_off, nslots;
  uint32_t rec_off, rec_cap;
  uint32_t gap_off, nlive;
  uint32_t free_head, hiwater;
  uint64_t num_streams;
  int64_t max_stream_id_bidi;
  uint64_t tx_goaway_id;
  uint32_t call;
  uint8_t ngaps, flags;
  int16_t err;
} qh_h3_smap;

typedef struct qh_h3_sent { /* 32 B */
  uint64_t stream_id;
  uint8_t pri_buf[8];
  uint32_t next;
  uint32_t call;
  uint16_t flags;
  uint8_t pri_len, rsv;
  uint32_t rsv2;
} qh_h3_sent;

typedef struct qh_h3_gap { /* 16 B */
  uint64_t begin, end;
} qh_h3_gap;

typedef struct qh_h3d_tab {
  qh_h3_smap *sm;
  size_t nconns;
  uint32_t *slots;
  uint64_t nslots;
  qh_h3_sent *ents;
  uint64_t nrecs;
  qh_h3_gap *gaps;
  uint64_t ngaps;
  qh_h3_stream *rs_pool;
  qh_http_state *hs_pool;
  qh_h3_uni *us_pool;
} qh_h3d_tab;

typedef struct qh_h3d_lists { /* dispatch's outputs, room for narrivals each */
  qh_span_in *b_chunks;
  uint8_t *b_fin;
  uint64_t *b_sid;
  uint32_t *b_view;
  uint32_t *b_rec;
  qh_h3_stream *rs_call;
  qh_http_state *hs_call;
  qh_span_in *u_chunks;
  uint8_t *u_fin;
  uint64_t *u_sid;
  uint32_t *u_rec;
  uint32_t *u_conn_start; /* nconns + 1 */
  qh_h3_uni *us_call;
} qh_h3d_lists;

/* 0, or QH_ERR_INVALID_ARGUMENT when a total passes 2^32 - 1. */
QH_EXPORT int qh_h3_smap_init(qh_h3_smap *sm, size_t n, int server, const uint32_t *rec_cap,
                              uint64_t totals[3]);

QH_EXPORT int qh_qpack_h3_dispatch(const qh_h3d_tab *t, const uint64_t *stream_id,
                                   const qh_span_in *chunks, const uint8_t *fin, size_t narrivals,
                                   const uint32_t *conn_start, int32_t *route, uint32_t *rec,
                                   const qh_h3d_lists *out, uint64_t *nbidi, uint64_t *nuni);
QH_EXPORT int qh_h3_dispatch_batch(qh_ctx *ctx, const qh_h3d_tab *t, const uint64_t *stream_id,
                                   const qh_span_in *chunks, const uint8_t *fin, size_t narrivals,
                                   const uint32_t *conn_start, int32_t *route, uint32_t *rec,
                                   const qh_h3d_lists *out, uint64_t *nbidi, uint64_t *nuni, int where);

QH_EXPORT int qh_qpack_h3_commit(const qh_h3d_tab *t, const uint32_t *b_rec,
                                 const qh_h3_stream *rs_call, const qh_http_state *hs_call,
                                 size_t nbidi, const uint32_t *u_rec, const qh_h3_uni *us_call,
                                 size_t nuni, uint32_t *nskipped);
QH_EXPORT int qh_h3_commit_batch(qh_ctx *ctx, const qh_h3d_tab *t, const uint32_t *b_rec,
                                 const qh_h3_stream *rs_call, const qh_http_state *hs_call,
                                 size_t nbidi, const uint32_t *u_rec, const qh_h3_uni *us_call,
                                 size_t nuni, uint32_t *nskipped, int where);

QH_EXPORT int qh_qpack_h3_open(const qh_h3d_tab *t, const qh_h3_conn *cs, const uint64_t *stream_id,
                               size_t n, const uint32_t *conn_start, int32_t *status, uint32_t *rec);
QH_EXPORT int qh_h3_open_batch(qh_ctx *ctx, const qh_h3d_tab *t, const qh_h3_conn *cs,
                               const uint64_t *stream_id, size_t n, const uint32_t *conn_start,
                               int32_t *status, uint32_t *rec, int where);

QH_EXPORT int qh_qpack_h3_find(const qh_h3d_tab *t, const uint32_t *conn, const uint64_t *stream_id,
                               size_t n, uint32_t *rec);
QH_EXPORT int qh_h3_find_batch(qh_ctx *ctx, const qh_h3d_tab *t, const uint32_t *conn,
                               const uint64_t *stream_id, size_t n, uint32_t *rec, int where);

QH_EXPORT int qh_qpack_h3_recs_move(void *pool, uint64_t npool, void *call, const uint32_t *idx,
                                    size_t n, uint32_t rec_bytes, int dir);
QH_EXPORT int qh_h3_recs_move_batch(qh_ctx *ctx, void *pool, uint64_t npool, void *call,
                                    const uint32_t *idx, size_t n, uint32_t rec_bytes, int dir,
                                    int where);

QH_EXPORT int qh_qpack_h3_close(const qh_h3d_tab *t, const uint64_t *stream_id, size_t n,
                                const uint32_t *conn_start, int32_t *status, uint64_t *cancel_sid,
                                uint32_t *cancel_view, uint64_t *ncancel, uint8_t *drained);
QH_EXPORT int qh_h3_close_batch(qh_ctx *ctx, const qh_h3d_tab *t, const uint64_t *stream_id, size_t n,
                                const uint32_t *conn_start, int32_t *status, uint64_t *cancel_sid,
                                uint32_t *cancel_view, uint64_t *ncancel, uint8_t *drained, int where);

QH_EXPORT int qh_qpack_h3_shutdown(const qh_h3d_tab *t, const uint32_t *csel, size_t nsel, int kind,
                                   uint64_t *goaway_id, int32_t *status);
QH_EXPORT int qh_h3_shutdown_batch(qh_ctx *ctx, const qh_h3d_tab *t, const uint32_t *csel, size_t nsel,
                                   int kind, uint64_t *goaway_id, int32_t *status, int where);

/* Library version string. */
QH_EXPORT const char *qh_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QHUFF_H */
