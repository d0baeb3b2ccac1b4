// modelfile_harness.cpp — the host half of csrc/ivit_modelfile.h (the reader and validator of model files) as a stand-alone program,
// so that it can be built with a plain host compiler and -fsanitize=address,undefined and run over good and corrupted files
// (tests/test_modelfile_cpu.py).  For every path in argv it prints one line, "<status>\t<message>", and the counts of a file that
// passed; the exit status is 0 whatever the files hold — a crash or a sanitizer report is what the test looks for.
#define IVIT_MODELFILE_HOST_ONLY
#include "../i-vit_amd/csrc/ivit_modelfile.h"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        ivit_model_info info;
        char msg[256];
        const int st = ivit_model_file_info(argv[i], &info, msg, sizeof(msg));
        if (st == IVIT_OK) printf("%d\tok kind %d records %d scalars %d blob %lld\n", st, info.kind, info.records, info.scalars, (long long)info.blob_bytes);
        else printf("%d\t%s\n", st, msg);
    }
    return 0;
}
