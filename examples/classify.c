/*
 * classify.c — a frozen model file run from plain C: no Python in the process.
 *
 *     classify model.ivit images.i8 B [k]
 *
 * model.ivit is a model file (include/ivit_modelfile.h: tools/freeze.py or engine.save wrote it), images.i8 holds B raw int8 images
 * [B, in_chans, img_size, img_size] already quantised at the model's input scale (ivit_model_info.s_input), k defaults to 5.  The
 * program opens the file (ivit_model_open: read, validate, upload, checksum on the device, ivit_*_create), runs ivit_vit_predict or
 * ivit_swin_predict with the file's "head.scale", and prints one line per image: its number, then k pairs class:value in the order
 * of ivit_logits_topk, the values with nine significant digits (enough to give back the float).
 *
 * Build (build() of __graft_entry__.py does this next to the library):
 *     cc -std=c11 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/classify.c -o classify \
 *        -Li-vit_amd/csrc -livit_hip -L/opt/rocm/lib -lamdhip64
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime_api.h>
#include "ivit.h"
#include "ivit_eval.h"
#include "ivit_modelfile.h"

static ivit_handle h;

static void die(const char *what, int st) {
    fprintf(stderr, "classify: %s: %s (%s)\n", what, ivit_status_string(st), h ? ivit_last_error(h) : "");
    exit(1);
}
#define IVIT(call) do { int st_ = (call); if (st_ != IVIT_OK) die(#call, st_); } while (0)
#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "classify: %s: %s\n", #call, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char **argv) {
    if (argc < 4 || argc > 5) {
        fprintf(stderr, "usage: classify model.ivit images.i8 B [k]   (library %d, eval %d, model files %d)\n", IVIT_VERSION, IVIT_EVAL_VERSION,
                IVIT_MODELFILE_VERSION);
        return 2;
    }
    const int B = atoi(argv[3]), k = argc == 5 ? atoi(argv[4]) : 5;
    if (B < 1 || k < 1) { fprintf(stderr, "classify: B and k must be positive\n"); return 2; }

    /* the file is checked on the host first: a bad file costs no device */
    ivit_model_info info;
    char msg[256];
    int st = ivit_model_file_info(argv[1], &info, msg, sizeof(msg));
    if (st != IVIT_OK) { fprintf(stderr, "classify: %s: %s (%s)\n", argv[1], ivit_status_string(st), msg); return 1; }

    const size_t per_image = (size_t)info.in_chans * info.img_size * info.img_size, nimg = per_image * (size_t)B;
    int8_t *images_host = (int8_t *)malloc(nimg);
    FILE *fp = fopen(argv[2], "rb");
    if (!images_host || !fp || fread(images_host, 1, nimg, fp) != nimg) {
        fprintf(stderr, "classify: %s: cannot read %d images of %zu bytes\n", argv[2], B, per_image);
        return 1;
    }
    fclose(fp);

    IVIT(ivit_create(&h, 0, NULL));
    ivit_model m = NULL;
    IVIT(ivit_model_open(h, argv[1], 1, &m));
    const void *head_scale = NULL;
    IVIT(ivit_model_constant(m, "head.scale", &head_scale, NULL));

    ivit_vit vit = NULL;
    ivit_swin swin = NULL;
    size_t ws_bytes = 0;
    if (info.kind == 1) {
        IVIT(ivit_model_vit(m, &vit));
        IVIT(ivit_vit_workspace_bytes(vit, B, 1, &ws_bytes));
    } else {
        IVIT(ivit_model_swin(m, &swin));
        IVIT(ivit_swin_workspace_bytes(swin, B, 1, &ws_bytes));
    }
    int8_t *images = NULL;
    void *ws = NULL;
    int32_t *logits = NULL, *idx = NULL;
    float *val = NULL;
    HIP(hipMalloc((void **)&images, nimg));
    HIP(hipMalloc(&ws, ws_bytes ? ws_bytes : 1));
    HIP(hipMalloc((void **)&logits, (size_t)B * info.num_classes * 4));
    HIP(hipMalloc((void **)&idx, (size_t)B * k * 4));
    HIP(hipMalloc((void **)&val, (size_t)B * k * 4));
    HIP(hipMemcpy(images, images_host, nimg, hipMemcpyHostToDevice));
    if (vit) {
        IVIT(ivit_vit_workspace_init(vit, ws, ws_bytes, B, 1));
        IVIT(ivit_vit_predict(vit, images, B, 1, ws, ws_bytes, logits, (const float *)head_scale, k, idx, val));
    } else {
        IVIT(ivit_swin_predict(swin, images, B, 1, ws, ws_bytes, logits, (const float *)head_scale, k, idx, val));
    }
    HIP(hipDeviceSynchronize());

    int32_t *idx_host = (int32_t *)malloc((size_t)B * k * 4);
    float *val_host = (float *)malloc((size_t)B * k * 4);
    if (!idx_host || !val_host) return 1;
    HIP(hipMemcpy(idx_host, idx, (size_t)B * k * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(val_host, val, (size_t)B * k * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        printf("%d", b);
        for (int j = 0; j < k; ++j) printf(" %d:%.9g", idx_host[b * k + j], val_host[b * k + j]);
        printf("\n");
    }

    free(idx_host); free(val_host); free(images_host);
    HIP(hipFree(val)); HIP(hipFree(idx)); HIP(hipFree(logits)); HIP(hipFree(ws)); HIP(hipFree(images));
    IVIT(ivit_model_close(m));
    IVIT(ivit_destroy(h));
    return 0;
}
