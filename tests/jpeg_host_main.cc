// A stand-alone driver of i-vit_amd/csrc/ivit_jpeg_host.h (no HIP, no Python): tests/test_jpeg_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and runs it over files of streams.
//
//   jpeg_host_main IN OUT
//
// IN:  per stream a little-endian uint32 length and the bytes.  OUT: per stream an int32 status; for IVIT_OK the eleven int32 w, h,
// ncomp, hs, vs, bw[3], bh[3], the 192 bytes of qt, an int64 count and the count int16 coefficients.  Every stream is copied into a
// heap block of exactly its length and decoded into a heap block of exactly the queried count, so that a read or a write outside
// either is the sanitizer's finding.  Exit status 0 when every stream was decoded or refused with IVIT_ERR_INVALID or
// IVIT_ERR_UNSUPPORTED and a reason; 1 otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../i-vit_amd/csrc/ivit_jpeg_host.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int bad = 0;
    long streams = 0, decoded = 0;
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t *exact = (uint8_t *)malloc(len ? len : 1);          // len == 0: one byte that is never to be read
        if (len && fread(exact, 1, len, in) != len) { fprintf(stderr, "short input\n"); return 2; }
        char err[128];
        ivit_jpeg_desc d;
        int64_t count = 0;
        size_t wsb = 0;
        int32_t st = ivit_jpeg_host_query(exact, len, &d, &count, &wsb, err, sizeof(err));
        int16_t *coefs = nullptr;
        if (st == IVIT_OK) {
            coefs = (int16_t *)malloc((size_t)count * 2);
            st = ivit_jpeg_host_entropy_decode(exact, len, coefs, count, err, sizeof(err));
            if (st == IVIT_OK && wsb != (size_t)count) { fprintf(stderr, "stream %ld: workspace bytes\n", streams); bad = 1; }
        }
        if (st != IVIT_OK && ((st != IVIT_ERR_INVALID && st != IVIT_ERR_UNSUPPORTED) || !err[0])) {
            fprintf(stderr, "stream %ld: status %d, reason `%s`\n", streams, st, err);
            bad = 1;
        }
        fwrite(&st, 4, 1, out);
        if (st == IVIT_OK) {
            const int32_t head[11] = {d.w, d.h, d.ncomp, d.hs, d.vs, d.bw[0], d.bw[1], d.bw[2], d.bh[0], d.bh[1], d.bh[2]};
            fwrite(head, 4, 11, out);
            fwrite(d.qt, 1, 192, out);
            fwrite(&count, 8, 1, out);
            fwrite(coefs, 2, (size_t)count, out);
            ++decoded;
        }
        free(coefs);
        free(exact);
        ++streams;
    }
    fclose(in);
    fclose(out);
    printf("%ld streams, %ld decoded, %ld refused\n", streams, decoded, streams - decoded);
    return bad;
}
