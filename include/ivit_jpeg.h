/*
 * ivit_jpeg.h — JPEG input: the Huffman entropy decode on the host, everything behind the coefficients (dequantisation, the inverse
 * DCT, chroma upsampling, YCbCr -> RGB, the crop to w x h) in ONE device call over a ragged batch, written straight into the `pixels`
 * pool that ivit_eval_transform_u8, ivit_view_transform_u8 and ivit_resize_center_crop_u8_pil read.  Thirteenth public header of
 * libivit_hip.so.
 *
 * Why a thirteenth header: ivit.h is frozen at IVIT_VERSION 111 and the eleven headers behind it at their versions 1 (their prototypes
 * and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header
 * includes ivit.h and uses its handle (ivit_handle), its status codes and its conventions: device pointers unless a name ends in
 * _host, asynchronous on the handle's HIP stream, nothing allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error
 * code; a pointer named in an "Alignment:" line is refused with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:"
 * line unless disjoint (ivit_last_error then contains "overlap" and both names), before anything is launched.  The two _host
 * entries take no handle and make no GPU call: their reason for a refusal goes to a caller-owned buffer.
 *
 * The definition: the bytes of Pillow's Image.open(f).convert("RGB"), every byte, no tolerance — libjpeg(-turbo)'s defaults: the
 * "islow" inverse DCT, "fancy" upsampling, its 16-bit fixed-point colour conversion.  ivit_amd/jpeg.py states both halves in numpy
 * (jpeg_coefficients_reference, jpeg_reference), DESIGN.md ("JPEG input") line by line, tests/golden/jpeg.npz — written by Pillow — is
 * the pin.  A stream is decoded to exactly those bytes or refused; nothing is approximated and no corrupt stream is repaired.
 *
 * Accepted: baseline and extended sequential Huffman streams (SOF0, SOF1) of 8-bit samples; one component (grey, whatever its
 * sampling factors: replicated to three channels), or three components that libjpeg's rule calls YCbCr (a JFIF marker; or an Adobe
 * marker with transform 1; or neither and component ids other than 'R', 'G', 'B') with luma 1x1, 2x1 or 2x2 and both chroma 1x1
 * (4:4:4, 4:2:2, 4:2:0); 8-bit quantisation tables; DHT / DQT redefinitions; DRI and RSTn; 0xFF fill bytes; APPn and COM segments;
 * bytes behind EOI; ONE interleaved scan.
 * IVIT_ERR_UNSUPPORTED, the message naming the reason: progressive (SOF2), arithmetic coding, lossless, hierarchical, 12-bit samples,
 * 4 components (CMYK / YCCK), RGB-coded files, other sampling factors, 16-bit quantisation tables, a sequential file of several scans,
 * DNL, and coefficients beyond what 8-bit samples give (the bound csrc/ivit_jpeg_host.h states: a column of a dequantised block whose
 * absolute values sum to more than 2950, or a sample outside [-512, 511] before the range limit).
 * IVIT_ERR_INVALID: every malformed or truncated stream (a bad length, a missing table, a Huffman code that is not in its table, a
 * run past coefficient 63, a restart marker out of sequence, data ending before the last MCU, no EOI behind it).
 *
 * Deliberately not here: progressive and arithmetic files; CMYK; EXIF orientation (Pillow's open does not apply it either);
 * device-side Huffman decoding; DCT-domain downscaling (Pillow's draft); PNG / WebP; encoding.
 */
#ifndef IVIT_JPEG_H
#define IVIT_JPEG_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_jpeg_query_host, ivit_jpeg_entropy_decode_host, ivit_jpeg_workspace_bytes, ivit_jpeg_reconstruct_u8. */
#define IVIT_JPEG_VERSION 1

/* One decoded file.  ivit_jpeg_query_host fills everything but the three offsets, which the caller sets when it places the file in
 * its batch.  Component c has bh[c] x bw[c] blocks (the MCU-padded grid): its coefficients are int16 [bh[c] * bw[c], 64], block-row-
 * major, natural order, component c behind component c - 1 from coef_offset; its plane in the workspace uint8 [bh[c] * 8, bw[c] * 8],
 * component after component from plane_offset. */
typedef struct ivit_jpeg_desc {
    int64_t coef_offset;       /* first coefficient of the file, in int16 ELEMENTS from `coefs`; a multiple of 8 */
    int64_t pixel_offset;      /* first byte of its h x w x 3 pixels in `pixels`: ivit_image_desc.offset */
    int64_t plane_offset;      /* first byte of its planes in `workspace`; a multiple of 16 */
    int32_t w, h;              /* 1 .. 65535 */
    int32_t ncomp;             /* 1 (grey) or 3 (YCbCr) */
    int32_t hs, vs;            /* luma sampling: 1x1, 2x1 or 2x2; 1x1 with one component */
    int32_t bw[3], bh[3];      /* blocks per row / column of every component; 0 for components that are not there */
    int32_t reserved;          /* 0 */
    uint8_t qt[192];           /* the components' quantisation tables, 64 each, natural order */
} ivit_jpeg_desc;              /* 264 bytes */

/* ---- v1  parses the headers of one file, data_host [bytes], up to its scan: *desc_host (offsets 0), *coef_count (int16 elements the
 * file decodes to) and *workspace_bytes (its planes); the last two may be NULL.  No GPU call, no allocation, nothing read outside the
 * range; thread-safe.  On a refusal err_host [err_bytes] (may be NULL) holds the reason, NUL-terminated.
 * Alignment: none.
 * Overlap: host memory only, desc_host, coef_count, workspace_bytes and err_host must not alias data_host (not checked). */
int ivit_jpeg_query_host(const uint8_t *data_host, size_t bytes, ivit_jpeg_desc *desc_host, int64_t *coef_count,
                         size_t *workspace_bytes, char *err_host, size_t err_bytes);

/* ---- v1  entropy-decodes one file into coefs_host [coef_capacity] int16 (pageable or pinned host memory): the *coef_count elements
 * of the query, zero where the stream codes nothing, DC prediction undone.  IVIT_ERR_INVALID if coef_capacity is smaller.  No GPU call,
 * no allocation, nothing written outside the first *coef_count elements and err_host; thread-safe for distinct outputs, so a host
 * decodes a batch on several threads.  On a refusal the coefficients are unspecified.
 * Alignment: coefs_host as int16.
 * Overlap: host memory only, coefs_host and err_host must not alias data_host (not checked). */
int ivit_jpeg_entropy_decode_host(const uint8_t *data_host, size_t bytes, int16_t *coefs_host, int64_t coef_capacity, char *err_host,
                                  size_t err_bytes);

/* ---- v1  *bytes = the workspace a batch needs when its files' planes lie back to back, each at a multiple of 16: the sum over the
 * B records of desc_host of their plane bytes rounded up to 16.  Reads bw, bh and ncomp only.  No GPU call.
 * Alignment: none.
 * Overlap: host memory only. */
int ivit_jpeg_workspace_bytes(const ivit_jpeg_desc *desc_host, int B, size_t *bytes);

/* ---- v1  the reconstruction of B decoded files of any sizes, samplings and tables: coefs int16 [coef_count] -> pixels, uint8 HWC,
 * h x w x 3 bytes at pixel_offset of every file, the definition above.  Two launches on the handle's stream: the IDCT of every block
 * into the planes of `workspace`, then upsampling, colour conversion and the crop.  No atomics, no workgroup waits for another, the
 * bytes do not depend on the grid.  desc_host and desc_dev are the SAME B records, on the host and on the device (the caller places
 * the device copy).  The call validates the host table before anything is launched — per file: w, h in 1 .. 65535; ncomp 1 or 3; hs x
 * vs 1x1, 2x1 or 2x2 (1x1 with one component); bw and bh what w, h and the sampling give; reserved 0; coef_offset >= 0, a multiple of
 * 8, and the file's coefficients inside coef_count; plane_offset >= 0, a multiple of 16, and the planes inside workspace_bytes;
 * pixel_offset >= 0 and the pixels inside pixels_bytes; and, so that no two files write the same byte, pixel_offset and plane_offset
 * of file i at or behind the end of file i - 1 — and returns IVIT_ERR_INVALID with the file's index in ivit_last_error ("image 3:
 * ...") otherwise.  The kernels read ONLY the device table: a replay of a captured graph reads it again, and may bring other
 * coefficients under the same descriptors (files of the same geometry and tables, or a table the caller rewrites between replays
 * within the captured launch shape).  Coefficients that break the host decoder's bound give unspecified BYTES (never an access
 * outside the buffers).  B >= 0; with B == 0 nothing is launched (every pointer may then be NULL).
 * Alignment: coefs and workspace 16 bytes, desc_dev 8 bytes, pixels none (byte stores).
 * Overlap: pixels (all pixels_bytes) and workspace (all workspace_bytes) may overlap neither each other, nor coefs, nor desc_dev:
 * IVIT_ERR_INVALID, nothing launched. */
int ivit_jpeg_reconstruct_u8(ivit_handle h, const int16_t *coefs, int64_t coef_count, const ivit_jpeg_desc *desc_host,
                             const ivit_jpeg_desc *desc_dev, int B, uint8_t *workspace, size_t workspace_bytes, uint8_t *pixels,
                             size_t pixels_bytes);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_JPEG_H */
