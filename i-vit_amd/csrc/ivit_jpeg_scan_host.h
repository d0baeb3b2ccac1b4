// ivit_jpeg_scan_host.h — the host pre-pass of include/ivit_jpeg_entropy.h: what of a file's entropy-coded data can be prepared
// without decoding a Huffman code.  Plain C++, no HIP, no allocation, no global state: a byte range in; a descriptor, a scan record
// with the tables in the device form, the unstuffed stream and its segments out.  It never reads outside [data, data + n) and never
// writes outside the capacities it was given; two calls with distinct outputs share nothing.  ivit_amd/jpeg.py
// (jpeg_scan_reference) states the stream and the segments in numpy; tests/jpeg_scan_main.cc runs this file alone, under the address
// and undefined-behaviour sanitizers too.
//
// The bytes behind SOS are read as libjpeg reads them (ivit_jpeg_host::Bits::fill): FF 00 is a data FF, FF FF .. FF 00 too (the fill
// FFs are dropped), FF x a marker.  A marker ends a segment.  Between segments only the RSTn the sequence asks for is taken, behind
// the last segment only EOI; what the host decoder would find out at those places (a restart marker out of sequence, no EOI, data
// that ends) is found here, so that the device kernel needs no marker at all: it gets whole bytes per segment and MCU counts.
#pragma once
#include "ivit_jpeg_host.h"
#include "../../include/ivit_jpeg_entropy.h"

namespace ivit_jpeg_host {

// the table selectors of the scan -> indices into two slots; false: a third table
static inline bool map_tables(const int sel[3], int ncomp, int slot_of[4], int out[3]) {
    int used = 0;
    for (int i = 0; i < 4; ++i) slot_of[i] = -1;
    for (int c = 0; c < 3; ++c) out[c] = 0;
    for (int c = 0; c < ncomp; ++c) {
        if (slot_of[sel[c]] < 0) {
            if (used == 2) return false;
            slot_of[sel[c]] = used++;
        }
        out[c] = slot_of[sel[c]];
    }
    return true;
}

static inline void emit_huff(const Huff &t, ivit_jpeg_huff *o) {
    memcpy(o->lut, t.lut, sizeof(o->lut));
    o->maxcode[0] = -1;
    o->mincode[0] = o->valptr[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        o->maxcode[l] = t.maxcode[l];
        o->mincode[l] = t.mincode[l];
        o->valptr[l] = t.valptr[l];
    }
    // the values the codes reach: valptr[16] + the codes of length 16 are at most 256
    int n = t.valptr[16] + (t.maxcode[16] >= 0 ? t.maxcode[16] - t.mincode[16] + 1 : 0);
    if (n > 256) n = 256;
    memset(o->vals, 0, sizeof(o->vals));
    memcpy(o->vals, t.vals, (size_t)n);
}

}  // namespace ivit_jpeg_host

static inline int ivit_jpeg_host_scan(const uint8_t *data, size_t bytes, ivit_jpeg_desc *desc, ivit_jpeg_scan *scan, uint8_t *stream,
                                      size_t stream_capacity, ivit_jpeg_segment *segments, int64_t segment_capacity, int64_t *coef_count,
                                      size_t *workspace_bytes, char *err, size_t err_bytes) {
    using namespace ivit_jpeg_host;
    Err e = {err, err_bytes};
    if (err && err_bytes) err[0] = 0;
    if (!data || !desc || !scan || !stream || !segments || segment_capacity < 0) return e.fail(IVIT_ERR_INVALID, "null argument");
    Stream s;
    if (const int st = parse(data, bytes, s, e)) return st;
    fill_desc(s, desc);
    if (coef_count) *coef_count = ivit_jpeg_host::coef_count(s);
    if (workspace_bytes) *workspace_bytes = plane_bytes(s.bw, s.bh, s.ncomp);
    memset(scan, 0, sizeof(*scan));
    int dslot[4], aslot[4], td[3], ta[3];
    if (!map_tables(s.td, s.ncomp, dslot, td)) return e.fail(IVIT_ERR_UNSUPPORTED, "more than two DC Huffman tables in one scan (device entropy decode)");
    if (!map_tables(s.ta, s.ncomp, aslot, ta)) return e.fail(IVIT_ERR_UNSUPPORTED, "more than two AC Huffman tables in one scan (device entropy decode)");
    for (int c = 0; c < 3; ++c) {
        scan->td[c] = td[c];
        scan->ta[c] = ta[c];
    }
    for (int i = 0; i < 4; ++i) {
        if (dslot[i] >= 0) emit_huff(s.dc[i], &scan->dc[dslot[i]]);
        if (aslot[i] >= 0) emit_huff(s.ac[i], &scan->ac[aslot[i]]);
    }
    scan->restart = s.restart;
    const int64_t total = (int64_t)s.mw * s.mh;
    const int64_t expected = s.restart ? (total + s.restart - 1) / s.restart : 1;
    if (expected > segment_capacity) return e.fail(IVIT_ERR_INVALID, "%lld segments, room for %lld", (long long)expected, (long long)segment_capacity);
    const uint8_t *p = data + s.scan, *end = data + bytes;
    size_t out = 0;
    int64_t seg = 0;
    for (;;) {                                       // one segment per round
        const size_t first = out;
        int marker = -1;                             // -1: the range ended
        while (p < end) {
            int c = *p++;
            if (c == 0xFF) {
                int x = 0xFF;
                while (p < end && (x = *p++) == 0xFF) {}
                if (x == 0xFF) break;                // FF .. FF up to the end of the range
                if (x != 0) { marker = x; break; }
            }
            if (out >= stream_capacity) return e.fail(IVIT_ERR_INVALID, "unstuffed stream: room for %zu bytes", stream_capacity);
            stream[out++] = (uint8_t)c;
        }
        ivit_jpeg_segment &g = segments[seg];
        g.bit_offset = (int64_t)first * 8;
        g.bit_count = (int64_t)(out - first) * 8;
        g.first_mcu = (int32_t)(seg * s.restart);
        g.mcu_count = (int32_t)(s.restart && (seg + 1) * s.restart <= total ? s.restart : total - seg * s.restart);
        if (marker < 0) return e.fail(IVIT_ERR_INVALID, "data ends before the last MCU");
        if (seg + 1 == expected) {
            if (marker != 0xD9) return e.fail(IVIT_ERR_INVALID, "no EOI behind the last MCU");
            break;
        }
        if (marker != 0xD0 + (int)(seg & 7)) return e.fail(IVIT_ERR_INVALID, "restart marker out of sequence");
        ++seg;
    }
    const size_t padded = (out + 7) & ~(size_t)7;
    if (padded > stream_capacity) return e.fail(IVIT_ERR_INVALID, "unstuffed stream: room for %zu bytes", stream_capacity);
    memset(stream + out, 0, padded - out);
    scan->stream_bytes = (int64_t)out;
    scan->segment_count = (int32_t)expected;
    return IVIT_OK;
}

// the per-file part of the device entry's workspace (include/ivit_jpeg_entropy.h): entry and exit state (8 bytes each) and a block
// count (4) per subsequence of the smallest size, and the first subsequence of every segment and the end (4 each)
#define IVIT_JPEG_ENTROPY_MAX_SUBSEQUENCES(stream_bytes, segment_count) ((stream_bytes) * 8 / IVIT_JPEG_ENTROPY_MIN_BITS + (segment_count) + 1)
static inline size_t ivit_jpeg_entropy_file_workspace(int64_t stream_bytes, int64_t segment_count) {
    const size_t n = (size_t)IVIT_JPEG_ENTROPY_MAX_SUBSEQUENCES(stream_bytes, segment_count) * 20 + (size_t)(segment_count + 1) * 4;
    return (n + 15) & ~(size_t)15;
}
