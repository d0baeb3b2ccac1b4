// A stand-alone driver of i-vit_amd/csrc/ivit_jpeg_scan_host.h (no HIP, no Python): tests/test_jpeg_entropy_cpu.py builds it twice,
// plain and with -fsanitize=address,undefined, and runs it as a child process.
//
//   jpeg_scan_main [--truncations] FILE...
//
// Per file one line: status, unstuffed bytes, segments, Adler-32 of the stream with its zero fill, Adler-32 of the segment records
// (zeros behind a refusal).  With --truncations every proper prefix of every file is scanned too and a line "prefixes N refused M"
// follows the file's.  Every input is copied into a heap block of exactly its length and scanned into heap blocks of exactly the
// capacities passed, so that a read or a write outside them is the sanitizer's finding.  Exit status 0 when every scan returned
// IVIT_OK or a refusal (IVIT_ERR_INVALID, IVIT_ERR_UNSUPPORTED) with a reason; 1 otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../i-vit_amd/csrc/ivit_jpeg_scan_host.h"

static uint32_t adler32(const uint8_t *p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) {
        a = (a + p[i]) % 65521;
        b = (b + a) % 65521;
    }
    return (b << 16) | a;
}

// 0 or a refusal: the status; -1: a status or a reason that must not be
static int scan_once(const uint8_t *data, size_t len, bool print) {
    uint8_t *exact = (uint8_t *)malloc(len ? len : 1);
    if (len) memcpy(exact, data, len);
    const int64_t cap = (int64_t)(len / 3 + 1);
    uint8_t *stream = (uint8_t *)malloc(len ? len : 1);
    ivit_jpeg_segment *segs = (ivit_jpeg_segment *)malloc((size_t)cap * sizeof(ivit_jpeg_segment));
    ivit_jpeg_desc d;
    ivit_jpeg_scan *rec = (ivit_jpeg_scan *)malloc(sizeof(ivit_jpeg_scan));
    char err[128];
    int64_t count = 0;
    size_t wsb = 0;
    int st = ivit_jpeg_host_scan(exact, len, &d, rec, stream, len, segs, cap, &count, &wsb, err, sizeof(err));
    if (st != IVIT_OK && ((st != IVIT_ERR_INVALID && st != IVIT_ERR_UNSUPPORTED) || !err[0])) {
        fprintf(stderr, "length %zu: status %d, reason `%s`\n", len, st, err);
        st = -1;
    }
    if (print) {
        if (st == IVIT_OK)
            printf("0 %lld %d %u %u\n", (long long)rec->stream_bytes, rec->segment_count, adler32(stream, (size_t)(rec->stream_bytes + 7) / 8 * 8),
                   adler32((const uint8_t *)segs, (size_t)rec->segment_count * sizeof(ivit_jpeg_segment)));
        else
            printf("%d 0 0 0 0\n", st);
    }
    free(rec);
    free(segs);
    free(stream);
    free(exact);
    return st;
}

int main(int argc, char **argv) {
    bool trunc = false;
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--truncations")) { trunc = true; continue; }
        FILE *in = fopen(argv[a], "rb");
        if (!in) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(in, 0, SEEK_END);
        const long len = ftell(in);
        fseek(in, 0, SEEK_SET);
        uint8_t *data = (uint8_t *)malloc(len > 0 ? (size_t)len : 1);
        if (len > 0 && fread(data, 1, (size_t)len, in) != (size_t)len) { fprintf(stderr, "short read of %s\n", argv[a]); return 2; }
        fclose(in);
        if (scan_once(data, (size_t)len, true) < 0) bad = 1;
        if (trunc) {
            long refused = 0;
            for (long n = 0; n < len; ++n) {
                const int st = scan_once(data, (size_t)n, false);
                if (st < 0) bad = 1;
                refused += st != IVIT_OK;
            }
            printf("prefixes %ld refused %ld\n", len, refused);
        }
        free(data);
    }
    return bad;
}
