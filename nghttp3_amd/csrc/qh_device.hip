// qh_device.hip -- QPACK Huffman batch engine for MI355X (gfx950, CDNA4).
//
// Replaces the hot loops of nghttp3's lib/nghttp3_qpack_huffman.c
// (encode_count :34-43, encode :45-78, decode :87-124) for batches of whole
// header-field strings.  Integer/byte work only: no MFMA.  Design notes and
// the roofline accounting are in DESIGN.md.
//
// Shipped kernels (all launched on the context's stream):
//   qh_k_dec_reserve + qh_k_dec_peek   decode, sorted 256-string windows, a
//                      W-bit table lookup per code (huffman.c:87-124)
//   qh_k_dec_reserve + qh_k_dec_peekw  decode, per-wave sorted chunks, input
//                      through LDS rings (QH_DECODER_WAVES)
//   qh_k_enc_lens_stream / _lane       encoded lengths (huffman.c:34-43)
//   qh_k_enc_lanes     codes, one string per lane, dense output through an
//                      LDS stage (huffman.c:45-78)
//   qh_k_frame_*, qh_k_sections_post, qh_k_check_fields,
//   qh_k_lookup_tokens QPACK framing, validation and tokens
//   qh_k_encsec_*      representation writer of whole field sections
//   qh_k_emit_*        field emission: index resolution, names and values gathered
//   qh_k_dts_*         encoder streams applied to many dynamic tables in one log
//   qh_k_encc_*        the encoder with inserts for many connections: walk and commit
//   qh_k_ack_*, qh_k_ackw_*  acknowledgements: the reference log, decoder streams read and written
//   qh_k_blk_*         blocked sections: queued, released, cancelled, compacted
//   qh_k_part_*        sections in pieces: held, reassembled at fin, compacted
//   qh_k_us_*          encoder and decoder streams as they arrive: cut instructions held
//   qh_k_http_*        decoded sections as HTTP messages: field verdicts, the kept records
//   qh_k_h3_*          request streams as they arrive: HTTP/3 frames cut, body accounting, settle
//   qh_k_h3w_*         streams as they leave: HTTP/3 frame headers written, payloads copied
//   qh_k_h3u_*         unidirectional streams as they arrive: types, control frames, SETTINGS
//   qh_k_h3d_*         streams by id: the per-connection stream table, arrivals routed, closes, GOAWAY ids
//   qh_k_idx_*         the hashed index over the views' keys: count, build
//   qh_k_scan, qh_k_synth_*   prefix sums, synthetic inputs (bench/tests)
// The kernels from qh_k_encsec_* to qh_k_http_* work a 16-lane group per table,
// connection or block and leave their totals in one scan header: both are
// qh_group.inc's.
// Development variants (the pair decoder, the segment encoder) build only
// with -DQH_DEV_VARIANTS (make dev -> libqhuff_dev.so); the kernels that
// exist only for them live outside the package, in dev/csrc (-I).  The older
// variants (fsm / fsm2 / lut / run / queue decoders, the chunk-engine and
// streaming encoders, the zero-copy host path) are in the history at 30ebdce.

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <condition_variable>
#include <atomic>
#include <thread>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/qhuff.h"
#include "qh_tables.h"
#include "qh_scratch.h"

#define QH_VERSION "0.2.0"

// One translation unit, split by concern:
#include "qh_common.h"      // span/stat types, tables, small helpers
#include "qh_chunk.inc"      // block ranges, windows, chunk rounds, scans
#include "qh_scan.inc"       // batch prefix sum (synthetic inputs)
#include "qh_group.inc"      // the state kernels' 16-lane group, the segmented scan's header
#include "qh_dec_common.inc"  // decode table blob, slot reservation
#include "qh_check.inc"       // field name / value checks (device)
#include "qh_sched.inc"       // batch-wide length-class schedule (QH_DECODER_SORTED)
#include "qh_peek_dec.inc"   // decoders (windows: default; waves): W-bit peek table + leading-ones table
#ifdef QH_DEV_VARIANTS         // development variants (make dev): not shipped
#include "qh_pair_dec.inc"   // (dev/csrc) decoder: two codes per lookup, waves fed from a group queue
#endif
#include "qh_lane_enc.inc"   // encoder: lengths (stream, lanes), codes (lanes: the default)
#include "qh_enc_waves.inc"   // encoder codes (QH_ENCODER_WAVES): per-wave chunks, LDS rings
#include "qh_enc_fused.inc"   // encoder, lengths + codes in one pass (QH_ENCODER_FUSED)
#include "qh_enc_region.inc"  // encoder codes over each window's region (QH_ENCODER_REGION, opt-in)
#ifdef QH_DEV_VARIANTS
#include "qh_enc_seg.inc"    // (dev/csrc) encoder, one pass over equal-size segments per lane
#endif
#include "qh_synth.inc"      // synthetic inputs for bench/tests
#include "qh_host.inc"   // host-memory decode: dense packing kernels
#include "qh_api.inc"    // host API (include/qhuff.h)
#include "qh_validate.inc"  // field name / value validation batch, header-name tokens
#include "qh_frame.inc"     // QPACK field-section framing on the device
#include "qh_sections.inc"  // whole field sections: frame -> decode -> fold / check / tokens
#include "qh_enc_sections.inc"  // whole field sections out: count -> pick -> encode -> write
#include "qh_emit.inc"          // decoded fields: resolve indices -> scan -> gather names and values
#include "qh_plan.inc"          // fields -> field lines (the encoder's static-table choice) -> sections
#include "qh_dyn_index.inc"     // a hashed index over the views' keys: count -> scan -> build
#include "qh_plan_dyn.inc"      // ... against a frozen dynamic table: keys, references, prefixes, scanned or through the index
#include "qh_dtset.inc"         // encoder streams of many connections -> dynamic tables in one log
#include "qh_encconn.inc"       // fields of many connections -> sections, encoder streams and tables, with inserts
#include "qh_ack.inc"           // acknowledgements: reference log, decoder streams read and written
#include "qh_blocked.inc"       // blocked sections: the queue log, push, release, cancel, compact
#include "qh_partial.inc"       // sections in pieces: held until fin, handed on whole; cancel, compact
#include "qh_ustream.inc"       // encoder and decoder streams as they arrive: cut instructions held; join, keep, sections, compact
#include "qh_httpmsg.inc"       // decoded sections as HTTP messages: fields kept, removed or malformed, the state per stream
#include "qh_h3.inc"            // request streams as they arrive: frames cut into HEADERS pieces and body spans; settle
#include "qh_h3w.inc"           // response and request streams as they leave: frames placed, headers written, payloads copied
#include "qh_h3u.inc"           // unidirectional streams as they arrive: types, control frames, SETTINGS; the peer's settings put to the encoders
#include "qh_h3d.inc"           // streams by id: a stream table per connection; arrivals routed to their records, opens, closes, GOAWAY ids
