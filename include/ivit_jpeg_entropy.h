/*
 * ivit_jpeg_entropy.h — JPEG input, the Huffman entropy decode on the device: a host pre-pass per file that needs no Huffman decoding
 * (parse, remove the byte stuffing, split at the RSTn markers, emit the tables), then ONE launch for a batch of B files that writes
 * the coefficients ivit_jpeg_reconstruct_u8 reads, and a verdict per file.  Fourteenth public header of libivit_hip.so.
 *
 * Why a fourteenth header: ivit.h is frozen at IVIT_VERSION 111 and the twelve headers behind it at their versions 1, ivit_jpeg.h
 * among them, so these entries are declared here, under a version of their own.  This header includes ivit_jpeg.h (and through it
 * ivit.h) and uses their handle, status codes, ivit_jpeg_desc and conventions: device pointers unless a name ends in _host,
 * asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error code; a
 * pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:" line
 * unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.  The _host entry takes no
 * handle and makes no GPU call.
 *
 * The definition: the coefficients ivit_jpeg_entropy_decode_host writes, every one, and its verdict per file; the accepted and the
 * refused streams are ivit_jpeg.h's.  One more refusal is this header's own: a scan that names more than two DC or more than two AC
 * Huffman tables (IVIT_ERR_UNSUPPORTED from ivit_jpeg_scan_host; baseline JPEG allows two of each, the host decoder takes four).
 *
 * The kernel (csrc/ivit_jpeg_entropy.h): one workgroup per file.  The file's tables lie in LDS; every lane owns subsequences of S
 * bits of the unstuffed stream and decodes them speculatively, the lanes exchange the decoder state (bit position, block of the MCU,
 * zigzag index) in which they cross into the next subsequence until nothing changes (Weissenberger and Schmidt's self-synchronising
 * decode, restated for JPEG's state), a prefix sum places every subsequence's blocks, a last decode writes the coefficients, a
 * segmented prefix sum undoes the DC prediction, and the host decoder's bound is checked per block.  No workgroup waits for another,
 * no atomics, the result does not depend on the grid or on S.  One file occupies ONE compute unit: a batch of 256 files fills the
 * device, a single very large file does not.
 *
 * Deliberately not here: progressive and arithmetic files (refused, as in ivit_jpeg.h); several workgroups per file; unstuffing on
 * the device (the pre-pass does it while it looks for the markers); a C batch helper with its own threads (ivit_jpeg_scan_host is
 * thread-safe for distinct outputs: the caller's pool runs it).
 */
#ifndef IVIT_JPEG_ENTROPY_H
#define IVIT_JPEG_ENTROPY_H

#include "ivit_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_jpeg_scan_host, ivit_jpeg_entropy_workspace_bytes, ivit_jpeg_entropy_decode. */
#define IVIT_JPEG_ENTROPY_VERSION 1

/* the smallest subsequence, in bits (a power of two); subsequence_bits == 0 selects the default (csrc/ivit_jpeg_entropy.h) */
#define IVIT_JPEG_ENTROPY_MIN_BITS 128

/* status[b] of ivit_jpeg_entropy_decode: 0, or the first refusal in stream order.  1 .. 5 are the host decoder's IVIT_ERR_INVALID
 * ("Huffman code not in the table", "run past coefficient 63", "DC coefficient outside 16 bits", "data ends before the last MCU",
 * "extraneous bytes before a marker"), 6 and 7 its IVIT_ERR_UNSUPPORTED ("coefficients beyond 8-bit samples": a column sum, a
 * sample). */
#define IVIT_JPEG_ENTROPY_BAD_CODE 1
#define IVIT_JPEG_ENTROPY_BAD_RUN 2
#define IVIT_JPEG_ENTROPY_BAD_DC 3
#define IVIT_JPEG_ENTROPY_DATA_ENDS 4
#define IVIT_JPEG_ENTROPY_EXTRANEOUS 5
#define IVIT_JPEG_ENTROPY_COLUMN_BOUND 6
#define IVIT_JPEG_ENTROPY_SAMPLE_BOUND 7

/* One entropy-coded segment (the data between two markers) of a file's unstuffed stream. */
typedef struct ivit_jpeg_segment {
    int64_t bit_offset;        /* its first bit, counted from the first byte of the FILE's stream; a multiple of 8 */
    int64_t bit_count;         /* its whole bytes, in bits: the up to 7 padding bits of the last byte included */
    int32_t first_mcu;         /* the MCU its first block belongs to: the MCUs of the segments before it */
    int32_t mcu_count;         /* the restart interval, less in the last segment; the whole image without DRI */
} ivit_jpeg_segment;           /* 24 bytes */

/* One Huffman table in the form the kernel copies into LDS: csrc/ivit_jpeg_host.h's Huff. */
typedef struct ivit_jpeg_huff {
    uint16_t lut[512];         /* 9 bits of look-ahead -> (length << 8) | symbol; 0: a longer code */
    int32_t maxcode[17];       /* the last code of length l, -1: none */
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
} ivit_jpeg_huff;              /* 1484 bytes */

/* One scanned file.  ivit_jpeg_scan_host fills everything but the three offsets, which the caller sets when it places the file in
 * its batch. */
typedef struct ivit_jpeg_scan {
    int64_t stream_offset;     /* first byte of its unstuffed stream in `streams`; a multiple of 16 */
    int64_t work_offset;       /* first byte of its part of `workspace`; a multiple of 16 */
    int64_t segment_offset;    /* its first record in `segments`, in RECORDS */
    int64_t stream_bytes;      /* unstuffed bytes; the stream is zero-filled up to the next multiple of 8, which belongs to it */
    int32_t segment_count;
    int32_t restart;           /* the restart interval in MCUs, 0: none */
    int32_t td[3], ta[3];      /* per component: which of dc[] / ac[] it uses, 0 or 1 */
    int32_t reserved[2];       /* 0 */
    ivit_jpeg_huff dc[2], ac[2];
} ivit_jpeg_scan;              /* 6008 bytes */

/* ---- v1  the host pre-pass of one file, data_host [bytes]: parses the headers (ivit_jpeg_query_host's refusals, statuses and
 * reasons), fills *desc_host (offsets 0) and *scan_host (offsets 0), copies the entropy-coded bytes to stream_host with the byte
 * stuffing removed (FF 00 -> FF, fill FFs dropped, markers left out) and zero-filled to a multiple of 8 bytes, and writes one
 * record per segment to segments_host.  The stream is never longer than the file: stream_capacity == bytes always suffices.  It checks
 * what needs no Huffman decoding: the RSTn markers are D0 .. D7 in order, the segments are as many as `restart` and the MCU count
 * give, EOI stands behind the last (IVIT_ERR_INVALID otherwise, as the host decoder refuses those files); IVIT_ERR_INVALID also when
 * a capacity is too small ("room for").  *coef_count and *workspace_bytes (may be NULL) are the query's.  No GPU call, no allocation,
 * nothing read outside the range, nothing written outside the capacities; thread-safe for distinct outputs.  On a refusal err_host
 * [err_bytes] (may be NULL) holds the reason and the outputs are unspecified.
 * Alignment: stream_host none, desc_host, scan_host and segments_host as their types.
 * Overlap: host memory only, no output may alias data_host or another output (not checked). */
int ivit_jpeg_scan_host(const uint8_t *data_host, size_t bytes, ivit_jpeg_desc *desc_host, ivit_jpeg_scan *scan_host, uint8_t *stream_host,
                        size_t stream_capacity, ivit_jpeg_segment *segments_host, int64_t segment_capacity, int64_t *coef_count,
                        size_t *workspace_bytes, char *err_host, size_t err_bytes);

/* ---- v1  *bytes = the workspace ivit_jpeg_entropy_decode needs for the B records of scan_host when the files' parts lie back to
 * back, each at a multiple of 16 (B == 1: the part of one file, the step to the next work_offset): per file 20 bytes per
 * subsequence of IVIT_JPEG_ENTROPY_MIN_BITS bits (stream_bytes / 16 + segment_count + 1 of them, whatever subsequence_bits the call
 * uses) and 4 per segment.  Reads stream_bytes and segment_count only.  No GPU call.
 * Alignment: none.
 * Overlap: host memory only. */
int ivit_jpeg_entropy_workspace_bytes(const ivit_jpeg_scan *scan_host, int B, size_t *bytes);

/* ---- v1  the entropy decode of B scanned files in one launch of B workgroups on the handle's stream: streams uint8
 * [streams_bytes] (every file's unstuffed stream at its stream_offset) -> coefs int16 [coef_count], in exactly the layout
 * ivit_jpeg_reconstruct_u8 reads (per file from desc.coef_offset: block-row-major per component, natural order, DC prediction undone,
 * zeros where nothing is coded; the kernel zeroes the file's range itself), and status int32 [B] (the codes above).  A refused
 * file's coefficients are unspecified; a refusal never touches another file's outputs.  desc_host / desc_dev, scan_host / scan_dev
 * and segments_host / segments_dev [segment_count records] are the SAME tables on the host and on the device (the caller places the
 * device copies).  The call validates the host copies before anything is launched — per file the descriptor as
 * ivit_jpeg_reconstruct_u8 does (the geometry, coef_offset and the coefficients inside coef_count); stream_offset >= 0, a multiple of
 * 16, and the stream with its zero fill inside streams_bytes, below 2^28 bytes; work_offset >= 0, a multiple of 16, and the file's
 * part inside workspace_bytes; the segments inside the table, ascending and inside the stream, their MCUs consecutive and summing to
 * the image's; td / ta 0 or 1, reserved 0; and stream_offset, work_offset and coef_offset of file i at or behind the end of file
 * i - 1 — and returns IVIT_ERR_INVALID with the file's index in ivit_last_error ("file 3: ...") otherwise.  The kernel reads ONLY the
 * device copies.  Whatever the stream's bytes say, no access leaves the file's stream, its coefficients, its part of the workspace
 * or the tables, and every loop is bounded by numbers of the records: a hostile stream ends with a nonzero status.
 * subsequence_bits: 0 (the default) or a power of two in IVIT_JPEG_ENTROPY_MIN_BITS .. 65536; the result does not depend on it.
 * B >= 0; with B == 0 nothing is launched (every pointer may then be NULL).  B <= 65535.
 * Alignment: streams, workspace and coefs 16 bytes, desc_dev, scan_dev and segments_dev 8 bytes, status 4 bytes.
 * Overlap: coefs (all coef_count elements), status (B elements) and workspace (all workspace_bytes) may overlap neither each other,
 * nor streams, nor desc_dev, scan_dev or segments_dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_jpeg_entropy_decode(ivit_handle h, const uint8_t *streams, size_t streams_bytes, const ivit_jpeg_desc *desc_host,
                             const ivit_jpeg_desc *desc_dev, const ivit_jpeg_scan *scan_host, const ivit_jpeg_scan *scan_dev,
                             const ivit_jpeg_segment *segments_host, const ivit_jpeg_segment *segments_dev, int64_t segment_count, int B,
                             int subsequence_bits, uint8_t *workspace, size_t workspace_bytes, int16_t *coefs, int64_t coef_count,
                             int32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_JPEG_ENTROPY_H */
