// ivit_jpeg_host.h — the host half of include/ivit_jpeg.h: a baseline JPEG parser and Huffman entropy decoder.  Plain C++, no HIP, no
// allocation, no global state: a byte range in, a descriptor and int16 coefficients out, a caller-owned buffer for the reason of a
// refusal.  It never reads outside [data, data + n), never writes outside the `capacity` coefficients (and the error buffer) it was
// given, and two calls with distinct outputs share nothing.  ivit_amd/jpeg.py (jpeg_coefficients_reference) states the same in numpy;
// tests/jpeg_host_main.cc runs this file alone, under the address and undefined-behaviour sanitizers too.
//
// What is taken and what is refused is include/ivit_jpeg.h's list.  Every malformed or truncated stream is IVIT_ERR_INVALID: there is
// no recovery from corrupt data, a file libjpeg decodes with a warning is refused.
//
// Output: per component a block-row-major array [bh * bw, 64] over the component's MCU-padded block grid, the quantised coefficients
// in natural (row-major, de-zigzagged) order, DC prediction undone; component c follows component c - 1.
//
// THE BOUND the device kernels rely on, enforced per block on the dequantised coefficients d = coefficient * quantiser:
//   (a) the absolute values of every COLUMN of the block sum to at most IVIT_JPEG_COLUMN_BOUND = 2950, and
//   (b) every sample of the block's inverse DCT, before the range limit, lies in [-512, 511].
// 8-bit samples give column sums of at most 8 * 1024 / sqrt(8) = 2897 and samples in [-128, 127] plus the quantiser's ringing; a
// stream that breaks either is IVIT_ERR_UNSUPPORTED.  (a) makes every multiplicand of the islow IDCT fit 16 bits after the column
// pass (2950 * 1.39 * 4 < 16384) and 24 bits where four of them are summed, so the 24-bit multiply is exact — and libjpeg-turbo's
// 16-bit SIMD forms compute what its C form computes.  (b) keeps the samples on the part of libjpeg's range-limit table where the
// C form (a 10-bit masked lookup that wraps around) and the SIMD forms (saturating packs) agree.  (b) is checked exactly: where the
// sum of all |d| of a block exceeds 2040 (4 * 510: below it no sample can leave the range) the block's IDCT is computed here.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/ivit_jpeg.h"

#define IVIT_JPEG_COLUMN_BOUND 2950
#define IVIT_JPEG_SUM_EXACT 2040

namespace ivit_jpeg_host {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    uint16_t lut[512];         // 9 bits of lookahead -> (length << 8) | symbol, 0: a longer code
    int32_t maxcode[17];       // the last code of length l, -1: none
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
};

struct Err {
    char *buf;
    size_t n;
    int fail(int status, const char *fmt, ...) const {
        if (buf && n) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, n, fmt, ap);
            va_end(ap);
        }
        return status;
    }
};

struct Stream {                // what the parser knows at the start of the scan
    int w, h, ncomp, hs, vs;
    int mw, mh;                // MCUs
    int bw[3], bh[3];
    uint8_t qt[3][64];         // natural order
    Huff dc[4], ac[4];
    int td[3], ta[3];
    int restart;
    size_t scan;               // the first entropy-coded byte
};

// jidctint.c's 1-D pass before the descale
static inline void islow8(const int32_t x[8], int32_t o[8]) {
    int32_t z1 = (x[2] + x[6]) * 4433;
    const int32_t e2 = z1 + x[6] * -15137, e3 = z1 + x[2] * 6270;
    const int32_t e0 = (x[0] + x[4]) * 8192, e1 = (x[0] - x[4]) * 8192;
    const int32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int32_t t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    int32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int32_t z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    o[0] = t10 + t3; o[7] = t10 - t3; o[1] = t11 + t2; o[6] = t11 - t2;
    o[2] = t12 + t1; o[5] = t12 - t1; o[3] = t13 + t0; o[4] = t13 - t0;
}

// the bound of the header comment on one block; d: dequantised, natural order.  0: inside, 1: (a) broken, 2: (b) broken
static inline int block_bound(const int32_t d[64], int *worst) {
    int total = 0;
    for (int c = 0; c < 8; ++c) {
        int s = 0;
        for (int r = 0; r < 8; ++r) s += d[r * 8 + c] < 0 ? -d[r * 8 + c] : d[r * 8 + c];
        if (s > IVIT_JPEG_COLUMN_BOUND) { *worst = s; return 1; }
        total += s;
    }
    if (total <= IVIT_JPEG_SUM_EXACT) return 0;
    int32_t ws[64], in[8], o[8];
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) in[r] = d[r * 8 + c];
        islow8(in, o);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = (o[r] + (1 << 10)) >> 11;
    }
    for (int r = 0; r < 8; ++r) {
        islow8(ws + r * 8, o);
        for (int c = 0; c < 8; ++c) {
            const int v = (o[c] + (1 << 17)) >> 18;
            if (v < -512 || v > 511) { *worst = v; return 2; }
        }
    }
    return 0;
}

static inline int build_huff(Huff &t, const uint8_t *counts, const uint8_t *vals, int nvals, bool dc, const Err &e) {
    memset(t.lut, 0, sizeof(t.lut));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return e.fail(IVIT_ERR_INVALID, "bad Huffman table: code lengths overflow");
            if (dc && vals[k] > 15) return e.fail(IVIT_ERR_INVALID, "bad Huffman table: DC category above 15");
            t.vals[k] = vals[k];
            if (l <= 9)
                for (int f = 0; f < (1 << (9 - l)); ++f) t.lut[(code << (9 - l)) | f] = (uint16_t)((l << 8) | vals[k]);
        }
        t.maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    (void)nvals;
    t.defined = true;
    return IVIT_OK;
}

static inline int parse(const uint8_t *d, size_t n, Stream &s, const Err &e) {
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return e.fail(IVIT_ERR_INVALID, "no SOI marker");
    size_t pos = 2;
    uint8_t qt[4][64];
    bool have_qt[4] = {false, false, false, false}, have_frame = false, jfif = false;
    int adobe = -1, cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    for (int i = 0; i < 4; ++i) s.dc[i].defined = s.ac[i].defined = false;
    s.restart = 0;
    s.ncomp = 0;
    for (;;) {
        if (pos >= n) return e.fail(IVIT_ERR_INVALID, "stream ends inside the headers");
        if (d[pos] != 0xFF) return e.fail(IVIT_ERR_INVALID, "marker expected");
        while (pos < n && d[pos] == 0xFF) ++pos;
        if (pos >= n) return e.fail(IVIT_ERR_INVALID, "stream ends inside the headers");
        const int m = d[pos++];
        if (m == 0xD9) return e.fail(IVIT_ERR_INVALID, "EOI before the image data");
        if (m == 0x00 || m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
            return e.fail(IVIT_ERR_INVALID, "marker 0x%02X where a segment is expected", m);
        if (pos + 2 > n) return e.fail(IVIT_ERR_INVALID, "stream ends inside the headers");
        const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
        if (L < 2 || pos + L > n) return e.fail(IVIT_ERR_INVALID, "bad segment length");
        const uint8_t *seg = d + pos + 2;
        const size_t len = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1) {
            if (have_frame) return e.fail(IVIT_ERR_INVALID, "two SOF markers");
            if (len < 6) return e.fail(IVIT_ERR_INVALID, "bad SOF length");
            if (seg[0] != 8) return e.fail(IVIT_ERR_UNSUPPORTED, "%d-bit samples (8-bit only)", seg[0]);
            const int nc = seg[5];
            s.h = (seg[1] << 8) | seg[2];
            s.w = (seg[3] << 8) | seg[4];
            if (len != 6 + 3 * (size_t)nc) return e.fail(IVIT_ERR_INVALID, "bad SOF length");
            if (s.h == 0 || s.w == 0) return e.fail(IVIT_ERR_INVALID, "empty image");
            if (nc == 4) return e.fail(IVIT_ERR_UNSUPPORTED, "4 components (CMYK / YCCK)");
            if (nc != 1 && nc != 3) return e.fail(IVIT_ERR_UNSUPPORTED, "%d components", nc);
            for (int i = 0; i < nc; ++i) {
                cid[i] = seg[6 + 3 * i];
                ch[i] = seg[7 + 3 * i] >> 4;
                cv[i] = seg[7 + 3 * i] & 15;
                tq[i] = seg[8 + 3 * i];
                if (ch[i] < 1 || ch[i] > 4 || cv[i] < 1 || cv[i] > 4 || tq[i] > 3) return e.fail(IVIT_ERR_INVALID, "bad component in SOF");
            }
            if (nc == 3 && (cid[0] == cid[1] || cid[0] == cid[2] || cid[1] == cid[2])) return e.fail(IVIT_ERR_INVALID, "duplicate component id");
            s.ncomp = nc;
            have_frame = true;
        } else if (m == 0xC2) {
            return e.fail(IVIT_ERR_UNSUPPORTED, "progressive JPEG (SOF2)");
        } else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
            return e.fail(IVIT_ERR_UNSUPPORTED, "lossless JPEG");
        } else if (m == 0xC9 || m == 0xCA || m == 0xCD || m == 0xCE || m == 0xCC) {
            return e.fail(IVIT_ERR_UNSUPPORTED, "arithmetic coding");
        } else if (m == 0xC5 || m == 0xC6 || m == 0xC8) {
            return e.fail(IVIT_ERR_UNSUPPORTED, "hierarchical JPEG");
        } else if (m == 0xDC) {
            return e.fail(IVIT_ERR_UNSUPPORTED, "DNL marker");
        } else if (m == 0xDB) {
            for (size_t i = 0; i < len; i += 65) {
                const int pq = seg[i] >> 4, t = seg[i] & 15;
                if (t > 3 || pq > 1) return e.fail(IVIT_ERR_INVALID, "bad DQT");
                if (pq == 1) return e.fail(IVIT_ERR_UNSUPPORTED, "16-bit quantisation table");
                if (i + 65 > len) return e.fail(IVIT_ERR_INVALID, "bad DQT length");
                for (int k = 0; k < 64; ++k) qt[t][kZigzag[k]] = seg[i + 1 + k];
                have_qt[t] = true;
            }
        } else if (m == 0xC4) {
            for (size_t i = 0; i < len;) {
                if (i + 17 > len) return e.fail(IVIT_ERR_INVALID, "bad DHT length");
                const int tc = seg[i] >> 4, th = seg[i] & 15;
                if (tc > 1 || th > 3) return e.fail(IVIT_ERR_INVALID, "bad DHT");
                int total = 0;
                for (int k = 0; k < 16; ++k) total += seg[i + 1 + k];
                if (total > 256 || i + 17 + (size_t)total > len) return e.fail(IVIT_ERR_INVALID, "bad DHT length");
                if (const int st = build_huff(tc == 0 ? s.dc[th] : s.ac[th], seg + i + 1, seg + i + 17, total, tc == 0, e)) return st;
                i += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (len != 2) return e.fail(IVIT_ERR_INVALID, "bad DRI length");
            s.restart = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0) {
            if (len >= 14 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (len >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
        } else if (m == 0xDA) {
            if (!have_frame) return e.fail(IVIT_ERR_INVALID, "SOS before SOF");
            const int nc = s.ncomp;
            if (len < 1 || len != 4 + 2 * (size_t)seg[0]) return e.fail(IVIT_ERR_INVALID, "bad SOS length");
            if (seg[0] != nc) return e.fail(IVIT_ERR_UNSUPPORTED, "a scan of %d of %d components (one interleaved scan only)", seg[0], nc);
            for (int i = 0; i < nc; ++i) {
                if (seg[1 + 2 * i] != cid[i]) return e.fail(IVIT_ERR_INVALID, "scan component out of order");
                s.td[i] = seg[2 + 2 * i] >> 4;
                s.ta[i] = seg[2 + 2 * i] & 15;
                if (s.td[i] > 3 || s.ta[i] > 3) return e.fail(IVIT_ERR_INVALID, "bad table selector in SOS");
                if (!s.dc[s.td[i]].defined || !s.ac[s.ta[i]].defined) return e.fail(IVIT_ERR_INVALID, "missing Huffman table");
            }
            if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0)
                return e.fail(IVIT_ERR_INVALID, "spectral selection in a sequential scan");
            if (nc == 3) {
                if (!jfif) {
                    if (adobe == 0) return e.fail(IVIT_ERR_UNSUPPORTED, "RGB-coded file (Adobe transform 0)");
                    if (adobe > 1) return e.fail(IVIT_ERR_UNSUPPORTED, "Adobe transform %d", adobe);
                    if (adobe < 0 && cid[0] == 0x52 && cid[1] == 0x47 && cid[2] == 0x42)
                        return e.fail(IVIT_ERR_UNSUPPORTED, "RGB-coded file (component ids R, G, B)");
                }
                const bool luma = (ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2);
                if (!luma || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1)
                    return e.fail(IVIT_ERR_UNSUPPORTED, "sampling factors %dx%d/%dx%d/%dx%d (4:4:4, 4:2:2 and 4:2:0 only)", ch[0], cv[0], ch[1],
                                  cv[1], ch[2], cv[2]);
                s.hs = ch[0];
                s.vs = cv[0];
            } else {
                s.hs = s.vs = 1;
            }
            for (int i = 0; i < nc; ++i) {
                if (!have_qt[tq[i]]) return e.fail(IVIT_ERR_INVALID, "missing quantisation table");
                memcpy(s.qt[i], qt[tq[i]], 64);
            }
            s.mw = (s.w + 8 * s.hs - 1) / (8 * s.hs);
            s.mh = (s.h + 8 * s.vs - 1) / (8 * s.vs);
            for (int i = 0; i < 3; ++i) {
                s.bw[i] = i < nc ? s.mw * (i == 0 ? s.hs : 1) : 0;
                s.bh[i] = i < nc ? s.mh * (i == 0 ? s.vs : 1) : 0;
            }
            s.scan = pos;
            return IVIT_OK;
        } else {
            return e.fail(IVIT_ERR_INVALID, "unknown marker 0x%02X", m);
        }
    }
}

static inline int64_t coef_count(const Stream &s) {
    int64_t n = 0;
    for (int i = 0; i < s.ncomp; ++i) n += (int64_t)s.bw[i] * s.bh[i] * 64;
    return n;
}

static inline void fill_desc(const Stream &s, ivit_jpeg_desc *out) {
    memset(out, 0, sizeof(*out));
    out->w = s.w;
    out->h = s.h;
    out->ncomp = s.ncomp;
    out->hs = s.hs;
    out->vs = s.vs;
    for (int i = 0; i < 3; ++i) {
        out->bw[i] = s.bw[i];
        out->bh[i] = s.bh[i];
    }
    for (int i = 0; i < s.ncomp; ++i) memcpy(out->qt + 64 * i, s.qt[i], 64);
}

// libjpeg's reading of entropy-coded bytes: FF 00 is a data FF, FF FF .. FF 00 too, FF x a marker, which ends the data.  Behind the
// data (a marker, the end of the range) the accumulator is fed zeros, counted in `pad`: cnt < pad says that a decoder consumed
// bits that are not there.
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc;
    int cnt, pad, marker;      // marker: 0 none yet, -1 the range ended, else the marker's code
    inline void fill() {
        while (cnt <= 48) {
            int c = 0;
            if (marker == 0) {
                if (p >= end) marker = -1;
                else {
                    c = *p++;
                    if (c == 0xFF) {
                        int x = 0xFF;
                        while (p < end && (x = *p++) == 0xFF) {}
                        if (x == 0xFF) { marker = -1; c = 0; }            // FF .. FF up to the end of the range
                        else if (x != 0) { marker = x; c = 0; }
                    }
                }
            }
            if (marker != 0) pad += 8;
            acc = (acc << 8) | (uint64_t)c;
            cnt += 8;
        }
    }
    inline int symbol(const Huff &t) {
        fill();
        const uint16_t hit = t.lut[(acc >> (cnt - 9)) & 511];
        if (hit) { cnt -= hit >> 8; return hit & 255; }
        const int code16 = (int)((acc >> (cnt - 16)) & 0xFFFF);
        for (int l = 10; l <= 16; ++l) {
            const int c = code16 >> (16 - l);
            if (c <= t.maxcode[l] && c >= t.mincode[l]) { cnt -= l; return t.vals[t.valptr[l] + c - t.mincode[l]]; }
        }
        return -1;
    }
    inline int bits(int s) {          // s in 1 .. 15, after symbol()
        cnt -= s;
        return (int)((acc >> cnt) & ((1u << s) - 1));
    }
    // the marker behind an entropy-coded segment: fewer than 8 real bits may be left (the padding of the last byte)
    inline int next_marker(const Err &e, int *m) {
        fill();
        if (cnt - pad >= 8) return e.fail(IVIT_ERR_INVALID, "extraneous bytes before a marker");
        if (marker <= 0) return e.fail(IVIT_ERR_INVALID, "data ends before the last MCU");
        *m = marker;
        acc = 0;
        cnt = pad = marker = 0;
        return IVIT_OK;
    }
};

// `out`: coef_count(s) elements, zeroed here
static inline int decode(const uint8_t *d, size_t n, const Stream &s, int16_t *out, const Err &e) {
    memset(out, 0, (size_t)coef_count(s) * sizeof(int16_t));
    int16_t *base[3];
    base[0] = out;
    for (int i = 1; i < 3; ++i) base[i] = base[i - 1] + (size_t)s.bw[i - 1] * s.bh[i - 1] * 64;
    Bits br = {d + s.scan, d + n, 0, 0, 0, 0};
    int pred[3] = {0, 0, 0}, next_rst = 0;
    const long long total = (long long)s.mw * s.mh;
    long long mcu = 0;
    for (int my = 0; my < s.mh; ++my) {
        for (int mx = 0; mx < s.mw; ++mx, ++mcu) {
            if (s.restart && mcu && mcu % s.restart == 0) {
                int m = 0;
                if (const int st = br.next_marker(e, &m)) return st;
                if (m != 0xD0 + next_rst) return e.fail(IVIT_ERR_INVALID, "restart marker out of sequence");
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < s.ncomp; ++c) {
                const int ch = c == 0 ? s.hs : 1, cv = c == 0 ? s.vs : 1;
                const Huff &dct = s.dc[s.td[c]], &act = s.ac[s.ta[c]];
                for (int by = 0; by < cv; ++by) {
                    for (int bx = 0; bx < ch; ++bx) {
                        int16_t *blk = base[c] + ((size_t)(my * cv + by) * s.bw[c] + (size_t)(mx * ch + bx)) * 64;
                        int32_t deq[64];
                        memset(deq, 0, sizeof(deq));
                        int sy = br.symbol(dct);
                        if (sy < 0) return e.fail(IVIT_ERR_INVALID, "Huffman code not in the table");
                        if (sy) {
                            const int v = br.bits(sy);
                            pred[c] += v >= (1 << (sy - 1)) ? v : v - (1 << sy) + 1;
                        }
                        if (pred[c] < -32768 || pred[c] > 32767) return e.fail(IVIT_ERR_INVALID, "DC coefficient outside 16 bits");
                        blk[0] = (int16_t)pred[c];
                        deq[0] = pred[c] * s.qt[c][0];
                        for (int k = 1; k < 64;) {
                            const int rs = br.symbol(act);
                            if (rs < 0) return e.fail(IVIT_ERR_INVALID, "Huffman code not in the table");
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz == 0) {
                                if (r != 15) break;
                                k += 16;
                                if (k > 64) return e.fail(IVIT_ERR_INVALID, "run past coefficient 63");
                                continue;
                            }
                            k += r;
                            if (k > 63) return e.fail(IVIT_ERR_INVALID, "run past coefficient 63");
                            const int v = br.bits(sz), nat = kZigzag[k];
                            const int val = v >= (1 << (sz - 1)) ? v : v - (1 << sz) + 1;
                            blk[nat] = (int16_t)val;
                            deq[nat] = val * s.qt[c][nat];
                            ++k;
                        }
                        if (br.cnt < br.pad) return e.fail(IVIT_ERR_INVALID, "data ends before the last MCU");
                        int worst = 0;
                        const int b = block_bound(deq, &worst);
                        if (b == 1)
                            return e.fail(IVIT_ERR_UNSUPPORTED, "coefficients beyond 8-bit samples: a block column sums to %d (bound %d)", worst,
                                          IVIT_JPEG_COLUMN_BOUND);
                        if (b == 2) return e.fail(IVIT_ERR_UNSUPPORTED, "coefficients beyond 8-bit samples: a sample of %d leaves the bound [-512, 511]", worst);
                    }
                }
            }
        }
    }
    (void)total;
    int m = 0;
    if (const int st = br.next_marker(e, &m)) return st;
    if (m != 0xD9) return e.fail(IVIT_ERR_INVALID, "no EOI behind the last MCU");
    return IVIT_OK;
}

// the planes of one image in the workspace: component after component, (bh * 8) rows of (bw * 8) bytes
static inline size_t plane_bytes(const int bw[3], const int bh[3], int ncomp) {
    size_t n = 0;
    for (int i = 0; i < ncomp; ++i) n += (size_t)bw[i] * bh[i] * 64;
    return n;
}

}  // namespace ivit_jpeg_host

// the two host entries of include/ivit_jpeg.h, as functions a stand-alone program can call too
static inline int ivit_jpeg_host_query(const uint8_t *data, size_t bytes, ivit_jpeg_desc *desc, int64_t *coef_count, size_t *workspace_bytes,
                                       char *err, size_t err_bytes) {
    ivit_jpeg_host::Err e = {err, err_bytes};
    if (err && err_bytes) err[0] = 0;
    if (!data || !desc) return e.fail(IVIT_ERR_INVALID, "null argument");
    ivit_jpeg_host::Stream s;
    if (const int st = ivit_jpeg_host::parse(data, bytes, s, e)) return st;
    ivit_jpeg_host::fill_desc(s, desc);
    if (coef_count) *coef_count = ivit_jpeg_host::coef_count(s);
    if (workspace_bytes) *workspace_bytes = ivit_jpeg_host::plane_bytes(s.bw, s.bh, s.ncomp);
    return IVIT_OK;
}

static inline int ivit_jpeg_host_entropy_decode(const uint8_t *data, size_t bytes, int16_t *coefs, int64_t coef_capacity, char *err,
                                                size_t err_bytes) {
    ivit_jpeg_host::Err e = {err, err_bytes};
    if (err && err_bytes) err[0] = 0;
    if (!data || !coefs) return e.fail(IVIT_ERR_INVALID, "null argument");
    ivit_jpeg_host::Stream s;
    if (const int st = ivit_jpeg_host::parse(data, bytes, s, e)) return st;
    if (ivit_jpeg_host::coef_count(s) > coef_capacity)
        return e.fail(IVIT_ERR_INVALID, "%lld coefficients, room for %lld", (long long)ivit_jpeg_host::coef_count(s), (long long)coef_capacity);
    return ivit_jpeg_host::decode(data, bytes, s, coefs, e);
}
