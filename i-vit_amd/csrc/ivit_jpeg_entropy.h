// ivit_jpeg_entropy.h — the device half of include/ivit_jpeg_entropy.h: the Huffman entropy decode of B scanned files, one workgroup
// of JENT_THREADS lanes per file, one launch.  What goes in is what csrc/ivit_jpeg_scan_host.h prepares (the unstuffed stream, whole
// bytes per segment, the tables); what comes out is what csrc/ivit_jpeg_host.h's decode() writes, and its verdict.
//
// A Huffman stream has no random access: where a symbol starts is known only behind the symbol before it.  But a decoder that starts
// at a wrong bit falls into step with the right one after a few symbols (the codes are self-synchronising in practice), and that is
// what makes the stream parallel (Weissenberger and Schmidt, "Massively parallel Huffman decoding on GPUs", ICPP 2018).  Here, with
// the state JPEG adds:
//
//   state      (p, c, k): the bit at which the next symbol starts, the block of the MCU it belongs to (which selects the tables) and the
//              zigzag index it codes (0: a DC symbol).  A symbol is a code and its extra bits: it is decoded where it STARTS.
//   subsequence  S bits of one segment, counted from the segment's first bit; a segment has at least one.  Subsequence i is decoded from
//              entry[i] up to the first symbol that starts at or behind its end: that state is exit[i], and cnt[i] the DC symbols
//              (blocks started) on the way.  Lane t owns subsequences t, t + JENT_THREADS, ...
//   rounds     entry[i] starts as (first bit of i, 0, 0) — for the first subsequence of a segment that IS the decoder's state — and
//              is marked dirty.  A round decodes every dirty subsequence; behind a barrier, every i whose exit[i] differs from
//              entry[i + 1] (in p, c OR k) replaces it and marks it dirty; a flag in LDS says whether anything changed.  By
//              induction from each segment's first subsequence the entries become the sequential decoder's; at most as many rounds
//              as the file has subsequences.  In these rounds a chain must not stop — a stopped chain cannot fall into step, and its
//              INVALID exit would travel down the segment one subsequence a round, just in front of the chain behind it — so a code
//              outside the table is taken as one bit and a run past coefficient 63 ends the block (a decoder out of step meets both);
//              in the write pass both are the refusals they are, and everything in front of the first refusal is the true decode.
//              Only a symbol that reaches past the segment's end has the exit INVALID: nothing follows it.
//   placement  an exclusive prefix sum over cnt gives every subsequence the index of its first block in scan order (from the segment's
//              first_mcu); the write pass decodes each subsequence once more, now with the block index, and stores every coefficient
//              through the zigzag table at its natural position in the component's block-row-major array — the DC DIFFERENCE in
//              place of the DC.  A segment is over when its MCUs are: the padding bits behind them are never parsed, 8 or more
//              bits left are a refusal, as are MCUs left without bits.
//   DC         a segmented prefix sum over the MCUs (every lane a run of consecutive MCUs, reset where an MCU index is a multiple of
//              the restart interval) turns the differences into coefficients and checks the 16-bit range.
//   bound      csrc/ivit_jpeg_host.h's THE BOUND per block, eight lanes a block in LDS as jpeg_idct_kernel has them: the column sums
//              against IVIT_JPEG_COLUMN_BOUND, and jpeg_islow8's two passes where the block's total exceeds IVIT_JPEG_SUM_EXACT.
//   verdict    every refusal carries (block in scan order) * 16 + code; the smallest of the file is the host decoder's first, since
//              everything in front of the first refusal is the true decode.  Reduced through LDS, no atomics.
//
// Untrusted bytes: a bit position is compared with the segment's end before a symbol is taken (words behind the stream read as 0 and
// are never loaded), k <= 63 and block < the segment's last block before a store, table indices are masked to the tables' sizes.
// Every loop runs at most S symbols, the subsequences, the segments (their logarithm), the MCUs or the blocks of the file — numbers of
// the records, not of the stream.
//
// The per-subsequence arrays lie in the caller's workspace (global memory: a large file has more subsequences than LDS holds), the
// tables, the scans' partial sums and the bound's blocks in LDS (about 43 KB).  One file occupies one compute unit.
#pragma once
#include "../../include/ivit_jpeg_entropy.h"
#include "ivit_jpeg.h"
#include "ivit_jpeg_scan_host.h"

#define JENT_THREADS 1024
#define JENT_WG_BLOCKS (JENT_THREADS / 8)
#define JENT_DEFAULT_BITS 512                            // the fastest of the sweep in profiles/README.md, "JPEG input"
#define JENT_HUFF_WORDS (4 * (int)sizeof(ivit_jpeg_huff) / 4)
#define JENT_NONE 0xFFFFFFFFu

typedef unsigned long long jent_state;                   // p: bits 0 .. 31, c: 32 .. 34, k: 35 .. 41
#define JENT_FIRST (1ull << 61)                          // entry only: the first subsequence of a segment
#define JENT_INVALID (1ull << 62)
#define JENT_DIRTY (1ull << 63)                          // entry only: to be decoded in the next round

// zigzag position -> natural position (ivit_jpeg_host::kZigzag, for the device)
static __device__ const unsigned char jent_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JentShared {
    ivit_jpeg_huff huff[4];                              // dc[0], dc[1], ac[0], ac[1]
    unsigned char zigzag[64];
    union {
        int4 scan[2][JENT_THREADS];
        int idct[JENT_WG_BLOCKS * JPEG_LDS_BLOCK];
        unsigned red[JENT_THREADS];
    };
    int changed;
};

// what a lane knows of its file, the same in every lane
struct JentFile {
    const unsigned *words;                               // the stream, big-endian bytes in 32-bit words
    unsigned nwords;
    long long stream_bits;
    short *coefs;                                        // the file's first coefficient
    int ncomp, hs, vs, nb, mw;                           // nb: blocks per MCU
    int bw0, bw1;
    long long n0, n1;                                    // blocks of component 0, 1
    int total_blocks;
    unsigned dsel, asel;                                 // bit comp: the DC / AC table of the component
    int S;
};

__device__ __forceinline__ int jent_comp(const JentFile &f, int j) { return f.ncomp == 1 || j < f.hs * f.vs ? 0 : j - f.hs * f.vs + 1; }

// the 64 coefficients of block b of the scan order; b in 0 .. total_blocks - 1
__device__ __forceinline__ short *jent_block(const JentFile &f, int b) {
    const int mcu = b / f.nb, j = b - mcu * f.nb, my = mcu / f.mw, mx = mcu - my * f.mw, comp = jent_comp(f, j);
    if (comp == 0) {
        const int by = j / f.hs, bx = j - by * f.hs;
        return f.coefs + ((long long)(my * f.vs + by) * f.bw0 + (mx * f.hs + bx)) * 64;
    }
    return f.coefs + (f.n0 + (comp == 2 ? f.n1 : 0) + (long long)my * f.bw1 + mx) * 64;
}

// exclusive prefix over the lanes of the workgroup, segmented: x, y, z are summed, w != 0 says that the lane's sums start anew (what
// came before it is dropped).  All lanes call it; *total: the inclusive value of the last lane.
__device__ __forceinline__ int4 jent_scan(JentShared &sh, int4 v, int4 *total) {
    const int t = threadIdx.x;
    int cur = 0;
    sh.scan[0][t] = v;
    __syncthreads();
    for (int d = 1; d < JENT_THREADS; d <<= 1) {
        int4 a = sh.scan[cur][t];
        if (t >= d && !a.w) {
            const int4 b = sh.scan[cur][t - d];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w = b.w;
        }
        sh.scan[cur ^ 1][t] = a;
        __syncthreads();
        cur ^= 1;
    }
    const int4 ex = t ? sh.scan[cur][t - 1] : make_int4(0, 0, 0, 0);
    *total = sh.scan[cur][JENT_THREADS - 1];
    __syncthreads();
    return ex;
}

// a[0 .. n) -> its exclusive prefix sums in place, every lane a run of consecutive elements; returns the total
__device__ __forceinline__ int jent_prefix_in_place(JentShared &sh, int *a, int n) {
    const int per = (n + JENT_THREADS - 1) / JENT_THREADS, i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += a[i];
    int4 total;
    int run = jent_scan(sh, make_int4(s, 0, 0, 0), &total).x;
    for (int i = i0; i < i1; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    __syncthreads();
    return total.x;
}

// the bits of segment s inside the stream, and how many subsequences they are
__device__ __forceinline__ void jent_segment(const JentFile &f, const ivit_jpeg_segment *seg, long long *begin, long long *end) {
    const long long b = min(max((long long)seg->bit_offset, 0ll), f.stream_bits);
    *begin = b;
    *end = min(max((long long)seg->bit_offset + (long long)seg->bit_count, b), f.stream_bits);
}
__device__ __forceinline__ int jent_subsequences(const JentFile &f, const ivit_jpeg_segment *seg) {
    long long b, e;
    jent_segment(f, seg, &b, &e);
    return max(1, (int)((e - b + f.S - 1) / f.S));
}

// the segment of subsequence i: the last s with first[s] <= i
__device__ __forceinline__ int jent_find_segment(const int *first, int nseg, int i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void jent_refuse(unsigned &err, int block, int code) { err = min(err, ((unsigned)block << 4) | (unsigned)code); }

// Decodes from `entry` every symbol that starts in front of sub_end; returns the state behind them (or JENT_INVALID) and in *started
// the DC symbols met.  WRITE: `blk` is the scan-order index of the next block to start, `last_blk` the end of the segment's blocks,
// `last_sub` says that sub_end is the segment's end; coefficients are stored and refusals recorded in err.
template <bool WRITE>
__device__ jent_state jent_decode(const JentShared &sh, const JentFile &f, jent_state entry, unsigned sub_end, unsigned seg_end, int *started,
                                  int blk, int last_blk, bool last_sub, unsigned &err) {
    unsigned p = (unsigned)entry;
    int c = (int)(entry >> 32) & 7, k = (int)(entry >> 35) & 127, n = 0;
    unsigned wi = p >> 5;
    unsigned long long acc = 0;
    int have = 0;
    auto word = [&](unsigned i) { return i < f.nwords ? __builtin_bswap32(f.words[i]) : 0u; };
    acc = ((unsigned long long)word(wi) << 32) << (p & 31);
    have = 32 - (int)(p & 31);
    ++wi;
    short *dst = nullptr;
    bool stopped = false;
    if (WRITE && k > 0) {
        if (blk < 1 || blk > last_blk) return JENT_INVALID;
        dst = jent_block(f, blk - 1);
    }
    for (int it = 0; it < f.S && p < sub_end; ++it) {
        const bool dc = k == 0;
        if (WRITE && dc && blk >= last_blk) { stopped = true; break; }
        if (have <= 32) {
            acc |= (unsigned long long)word(wi++) << (32 - have);
            have += 32;
        }
        const int comp = jent_comp(f, c);
        const ivit_jpeg_huff &t = sh.huff[dc ? ((f.dsel >> comp) & 1) : 2 + ((f.asel >> comp) & 1)];
        const int code16 = (int)(acc >> 48);
        const unsigned hit = t.lut[code16 >> 7];
        int len = min((int)(hit >> 8), 16), sym = hit & 255;
        if (!hit) {
            len = 0;
            for (int l = 10; l <= 16; ++l) {
                const int cc = code16 >> (16 - l);
                if (cc <= t.maxcode[l] && cc >= t.mincode[l]) {
                    len = l;
                    sym = t.vals[(t.valptr[l] + cc - t.mincode[l]) & 255];
                    break;
                }
            }
        }
        const int bad_at = dc ? blk : blk - 1;
        if (len == 0) {
            if (!WRITE) {
                len = 1;                                     // speculation goes on, a bit further: see "rounds" above
                sym = 0;
            } else {
                jent_refuse(err, bad_at, IVIT_JPEG_ENTROPY_BAD_CODE);
                *started = n;
                return JENT_INVALID;
            }
        }
        const int sz = sym & 15, r = dc ? 0 : sym >> 4;
        if (p + (unsigned)(len + sz) > seg_end) {
            if (WRITE) jent_refuse(err, bad_at, IVIT_JPEG_ENTROPY_DATA_ENDS);
            *started = n;
            return JENT_INVALID;
        }
        int val = 0;
        if (sz) {
            const int v = (int)((acc << len) >> (64 - sz));
            val = v >= (1 << (sz - 1)) ? v : v - (1 << sz) + 1;
        }
        acc <<= len + sz;
        have -= len + sz;
        p += (unsigned)(len + sz);
        if (dc) {
            ++n;
            if (WRITE) {
                dst = jent_block(f, blk);
                ++blk;
                dst[0] = (short)val;
            }
            k = 1;
        } else if (sz == 0) {
            k = r == 15 ? k + 16 : 64;
            if (k > 64) {
                if (!WRITE) {
                    k = 64;                                  // speculation goes on: see "rounds" above
                } else {
                    jent_refuse(err, bad_at, IVIT_JPEG_ENTROPY_BAD_RUN);
                    *started = n;
                    return JENT_INVALID;
                }
            }
        } else {
            k += r;
            if (k > 63) {
                if (!WRITE) {
                    k = 63;
                } else {
                    jent_refuse(err, bad_at, IVIT_JPEG_ENTROPY_BAD_RUN);
                    *started = n;
                    return JENT_INVALID;
                }
            }
            if (WRITE) dst[sh.zigzag[k]] = (short)val;
            ++k;
        }
        if (k >= 64) {
            k = 0;
            c = c + 1 >= f.nb ? 0 : c + 1;
        }
    }
    *started = n;
    if (WRITE) {
        if (stopped) {                                       // the segment's MCUs are done: the padding of one byte may be left
            if (seg_end - p >= 8) jent_refuse(err, last_blk, IVIT_JPEG_ENTROPY_EXTRANEOUS);
        } else if (p < sub_end) {                            // S symbols without S bits: a table no header gives
            jent_refuse(err, k ? blk - 1 : blk, IVIT_JPEG_ENTROPY_BAD_CODE);
            return JENT_INVALID;
        } else if (last_sub && (blk < last_blk || k != 0)) {
            jent_refuse(err, k ? blk - 1 : blk, IVIT_JPEG_ENTROPY_DATA_ENDS);
        }
    }
    return (jent_state)p | ((jent_state)c << 32) | ((jent_state)k << 35);
}

__device__ __forceinline__ void jent_add(int &a, int &b, int &c, int comp, int v) {
    if (comp == 0) a += v; else if (comp == 1) b += v; else c += v;
}

__global__ __launch_bounds__(JENT_THREADS) void jpeg_entropy_kernel(const unsigned char *__restrict__ streams, const ivit_jpeg_desc *__restrict__ desc,
                                                                    const ivit_jpeg_scan *__restrict__ scan, const ivit_jpeg_segment *__restrict__ segments,
                                                                    int S, unsigned char *__restrict__ workspace, short *__restrict__ coefs,
                                                                    int *__restrict__ status) {
    __shared__ JentShared sh;
    const int t = threadIdx.x;
    const ivit_jpeg_desc *d = desc + blockIdx.x;
    const ivit_jpeg_scan *sc = scan + blockIdx.x;
    {
        const unsigned *src = reinterpret_cast<const unsigned *>(sc->dc);
        unsigned *dst = reinterpret_cast<unsigned *>(sh.huff);
        for (int i = t; i < JENT_HUFF_WORDS; i += JENT_THREADS) dst[i] = src[i];
        if (t < 64) sh.zigzag[t] = jent_zigzag[t];
    }
    JentFile f;
    f.ncomp = d->ncomp; f.hs = d->hs; f.vs = d->vs;
    f.nb = f.ncomp == 3 ? f.hs * f.vs + 2 : 1;
    f.bw0 = d->bw[0]; f.bw1 = d->bw[1];
    f.mw = f.bw0 / f.hs;
    f.n0 = (long long)d->bw[0] * d->bh[0];
    f.n1 = f.ncomp == 3 ? (long long)d->bw[1] * d->bh[1] : 0;
    f.total_blocks = (int)(f.n0 + 2 * f.n1);
    f.coefs = coefs + d->coef_offset;
    f.words = reinterpret_cast<const unsigned *>(streams + sc->stream_offset);
    f.nwords = (unsigned)((sc->stream_bytes + 7) / 8 * 2);
    f.stream_bits = sc->stream_bytes * 8;
    f.dsel = (unsigned)(sc->td[0] | (sc->td[1] << 1) | (sc->td[2] << 2));
    f.asel = (unsigned)(sc->ta[0] | (sc->ta[1] << 1) | (sc->ta[2] << 2));
    f.S = S;
    const int total_mcus = f.mw * (d->bh[0] / f.vs), nseg = sc->segment_count, restart = sc->restart;
    const ivit_jpeg_segment *segs = segments + sc->segment_offset;
    const int maxsub = (int)IVIT_JPEG_ENTROPY_MAX_SUBSEQUENCES((long long)sc->stream_bytes, nseg);
    jent_state *entry = reinterpret_cast<jent_state *>(workspace + sc->work_offset), *exits = entry + maxsub;
    int *cnt = reinterpret_cast<int *>(exits + maxsub), *first = cnt + maxsub;     // first: nseg + 1 elements
    unsigned err = JENT_NONE;

    // zeros where nothing is coded
    for (long long i = t; i < (long long)f.total_blocks * 8; i += JENT_THREADS) reinterpret_cast<int4 *>(f.coefs)[i] = make_int4(0, 0, 0, 0);
    // the first subsequence of every segment
    for (int s = t; s < nseg; s += JENT_THREADS) first[s] = jent_subsequences(f, segs + s);
    __syncthreads();
    const int nsub = min(jent_prefix_in_place(sh, first, nseg), maxsub);
    if (t == 0) first[nseg] = nsub;
    __syncthreads();
    for (int i = t; i < nsub; i += JENT_THREADS) {
        const int s = jent_find_segment(first, nseg, i);
        long long b, e;
        jent_segment(f, segs + s, &b, &e);
        entry[i] = (jent_state)(unsigned)(b + (long long)(i - first[s]) * S) | JENT_DIRTY | (i == first[s] ? JENT_FIRST : 0);
    }
    __syncthreads();

    // the rounds
    for (int round = 0; round <= nsub; ++round) {
        for (int i = t; i < nsub; i += JENT_THREADS) {
            const jent_state e = entry[i];
            if (!(e & JENT_DIRTY)) continue;
            entry[i] = e & ~JENT_DIRTY;
            int n = 0;
            jent_state x = JENT_INVALID;
            if (!(e & JENT_INVALID)) {
                const int s = jent_find_segment(first, nseg, i);
                long long b, end;
                jent_segment(f, segs + s, &b, &end);
                const long long sub_end = min(end, b + (long long)(i - first[s] + 1) * S);
                x = jent_decode<false>(sh, f, e, (unsigned)sub_end, (unsigned)end, &n, 0, 0, false, err);
            }
            exits[i] = x;
            cnt[i] = n;
        }
        if (t == 0) sh.changed = 0;
        __syncthreads();
        for (int i = t; i + 1 < nsub; i += JENT_THREADS) {
            const jent_state next = entry[i + 1], x = exits[i];
            if (!(next & JENT_FIRST) && next != x) {
                entry[i + 1] = x | JENT_DIRTY;
                sh.changed = 1;
            }
        }
        __syncthreads();
        const int again = sh.changed;
        __syncthreads();
        if (!again) break;
    }

    // placement and the write pass
    jent_prefix_in_place(sh, cnt, nsub);
    for (int i = t; i < nsub; i += JENT_THREADS) {
        const jent_state e = entry[i];
        if (e & (JENT_INVALID | JENT_DIRTY)) continue;
        const int s = jent_find_segment(first, nseg, i);
        long long b, end;
        jent_segment(f, segs + s, &b, &end);
        const long long sub_end = min(end, b + (long long)(i - first[s] + 1) * S);
        const long long seg_blk = (long long)segs[s].first_mcu * f.nb, seg_last = seg_blk + (long long)segs[s].mcu_count * f.nb;
        const int last_blk = (int)min(max(seg_last, 0ll), (long long)f.total_blocks);
        const long long blk = seg_blk + (cnt[i] - cnt[first[s]]);
        if (seg_blk < 0 || blk < seg_blk || blk > last_blk) continue;
        int n = 0;
        jent_decode<true>(sh, f, e, (unsigned)sub_end, (unsigned)end, &n, (int)blk, last_blk, i + 1 == first[s + 1], err);
    }
    __syncthreads();

    // DC prediction: every lane a run of consecutive MCUs
    {
        const int per = (total_mcus + JENT_THREADS - 1) / JENT_THREADS, m0 = min(total_mcus, t * per), m1 = min(total_mcus, m0 + per);
        int a = 0, b = 0, c = 0, reset = 0;
        for (int m = m0; m < m1; ++m) {
            if (restart > 0 && m % restart == 0) { a = b = c = 0; reset = 1; }
            for (int j = 0; j < f.nb; ++j) jent_add(a, b, c, jent_comp(f, j), jent_block(f, m * f.nb + j)[0]);
        }
        int4 total;
        const int4 in = jent_scan(sh, make_int4(a, b, c, reset), &total);
        a = in.x; b = in.y; c = in.z;
        for (int m = m0; m < m1; ++m) {
            if (restart > 0 && m % restart == 0) a = b = c = 0;
            for (int j = 0; j < f.nb; ++j) {
                const int comp = jent_comp(f, j);
                short *blk = jent_block(f, m * f.nb + j);
                jent_add(a, b, c, comp, blk[0]);
                const int pred = comp == 0 ? a : comp == 1 ? b : c;
                if (pred < -32768 || pred > 32767) jent_refuse(err, m * f.nb + j, IVIT_JPEG_ENTROPY_BAD_DC);
                blk[0] = (short)pred;
            }
        }
    }
    __syncthreads();

    // the bound, eight lanes a block
    {
        const int sub = t >> 3, l = t & 7;
        int *w = sh.idct + sub * JPEG_LDS_BLOCK;
        for (int base = 0; base < f.total_blocks; base += JENT_WG_BLOCKS) {
            const int g = base + sub;
            const bool active = g < f.total_blocks;
            int comp = 0;
            long long inner = g;
            int4 raw = make_int4(0, 0, 0, 0);
            uint2 q = make_uint2(0, 0);
            if (active) {
                if (g >= f.n0 + f.n1) { comp = 2; inner = g - f.n0 - f.n1; }
                else if (g >= f.n0) { comp = 1; inner = g - f.n0; }
                raw = *reinterpret_cast<const int4 *>(f.coefs + (long long)g * 64 + l * 8);
                q = *reinterpret_cast<const uint2 *>(d->qt + comp * 64 + l * 8);
            }
            int *row = w + l * JPEG_LDS_ROW;
            row[0] = (int)(short)(raw.x & 0xFFFF) * (int)(q.x & 255);
            row[1] = (raw.x >> 16) * (int)((q.x >> 8) & 255);
            row[2] = (int)(short)(raw.y & 0xFFFF) * (int)((q.x >> 16) & 255);
            row[3] = (raw.y >> 16) * (int)(q.x >> 24);
            row[4] = (int)(short)(raw.z & 0xFFFF) * (int)(q.y & 255);
            row[5] = (raw.z >> 16) * (int)((q.y >> 8) & 255);
            row[6] = (int)(short)(raw.w & 0xFFFF) * (int)((q.y >> 16) & 255);
            row[7] = (raw.w >> 16) * (int)(q.y >> 24);
            __syncthreads();
            int x[8], o[8], s = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                x[r] = w[r * JPEG_LDS_ROW + l];
                s += abs(x[r]);
            }
            int sum = s;
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 4);
            // the block's index in scan order, for the verdict
            int scan_blk = 0;
            if (active) {
                if (comp == 0) {
                    const int by = (int)(inner / f.bw0), bx = (int)(inner - (long long)by * f.bw0);
                    scan_blk = ((by / f.vs) * f.mw + bx / f.hs) * f.nb + (by % f.vs) * f.hs + bx % f.hs;
                } else {
                    scan_blk = (int)inner * f.nb + f.hs * f.vs + comp - 1;
                }
            }
            if (s > IVIT_JPEG_COLUMN_BOUND) jent_refuse(err, scan_blk, IVIT_JPEG_ENTROPY_COLUMN_BOUND);
            const bool exact = sum > IVIT_JPEG_SUM_EXACT;
            if (exact) {
                jpeg_islow8(x, o);
#pragma unroll
                for (int r = 0; r < 8; ++r) w[r * JPEG_LDS_ROW + l] = (o[r] + (1 << 10)) >> 11;
            }
            __syncthreads();
            if (exact) {
#pragma unroll
                for (int c = 0; c < 8; ++c) x[c] = w[l * JPEG_LDS_ROW + c];
                jpeg_islow8(x, o);
                bool out = false;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int v = (o[c] + (1 << 17)) >> 18;
                    out |= v < -512 || v > 511;
                }
                if (out) jent_refuse(err, scan_blk, IVIT_JPEG_ENTROPY_SAMPLE_BOUND);
            }
            __syncthreads();
        }
    }

    // the verdict: the smallest key of the workgroup
    sh.red[t] = err;
    __syncthreads();
    for (int dlt = JENT_THREADS / 2; dlt > 0; dlt >>= 1) {
        if (t < dlt) sh.red[t] = min(sh.red[t], sh.red[t + dlt]);
        __syncthreads();
    }
    if (t == 0) status[blockIdx.x] = sh.red[0] == JENT_NONE ? 0 : (int)(sh.red[0] & 15);
}
