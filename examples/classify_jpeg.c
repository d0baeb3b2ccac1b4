/*
 * classify_jpeg.c — from a JPEG file to the top-k classes of a frozen model in plain C: no Python in the process, no image library.
 *
 *     classify_jpeg model.ivit file.jpg [k]
 *
 * model.ivit is a model file (include/ivit_modelfile.h), k defaults to 5.  The program parses and entropy-decodes the file on the host
 * (ivit_jpeg_query_host, ivit_jpeg_entropy_decode_host: include/ivit_jpeg.h), reconstructs its pixels on the device
 * (ivit_jpeg_reconstruct_u8: Pillow's bytes), takes them through the reference's eval transform (ivit_eval_transform_u8: resize the
 * shorter side to int(img_size / 0.875), centre crop, normalise, quantise at the file's input scale) and runs ivit_vit_predict or
 * ivit_swin_predict.  It prints one line: 0, then k pairs class:value in the order of ivit_logits_topk, the values with nine
 * significant digits.  A file the decoder refuses is reported with the library's reason and exit status 1.
 *
 * Build (build() of __graft_entry__.py does this next to the library):
 *     cc -std=c11 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/classify_jpeg.c -o classify_jpeg \
 *        -Li-vit_amd/csrc -livit_hip -L/opt/rocm/lib -lamdhip64
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime_api.h>
#include "ivit.h"
#include "ivit_eval.h"
#include "ivit_modelfile.h"
#include "ivit_jpeg.h"

static ivit_handle h;

static void die(const char *what, int st) {
    fprintf(stderr, "classify_jpeg: %s: %s (%s)\n", what, ivit_status_string(st), h ? ivit_last_error(h) : "");
    exit(1);
}
#define IVIT(call) do { int st_ = (call); if (st_ != IVIT_OK) die(#call, st_); } while (0)
#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "classify_jpeg: %s: %s\n", #call, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char **argv) {
    if (argc < 3 || argc > 4) {
        fprintf(stderr, "usage: classify_jpeg model.ivit file.jpg [k]   (library %d, model files %d, jpeg %d)\n", IVIT_VERSION,
                IVIT_MODELFILE_VERSION, IVIT_JPEG_VERSION);
        return 2;
    }
    const int k = argc == 4 ? atoi(argv[3]) : 5;
    if (k < 1) { fprintf(stderr, "classify_jpeg: k must be positive\n"); return 2; }

    ivit_model_info info;
    char msg[256];
    int st = ivit_model_file_info(argv[1], &info, msg, sizeof(msg));
    if (st != IVIT_OK) { fprintf(stderr, "classify_jpeg: %s: %s (%s)\n", argv[1], ivit_status_string(st), msg); return 1; }
    if (info.in_chans != 3) { fprintf(stderr, "classify_jpeg: the model takes %d channels, a decoded file has 3\n", info.in_chans); return 1; }

    /* the file, parsed and entropy-decoded on the host: no device yet */
    FILE *fp = fopen(argv[2], "rb");
    long file_bytes = 0;
    if (!fp || fseek(fp, 0, SEEK_END) != 0 || (file_bytes = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0) {
        fprintf(stderr, "classify_jpeg: %s: cannot read\n", argv[2]);
        return 1;
    }
    uint8_t *file = (uint8_t *)malloc(file_bytes ? (size_t)file_bytes : 1);
    if (!file || fread(file, 1, (size_t)file_bytes, fp) != (size_t)file_bytes) { fprintf(stderr, "classify_jpeg: %s: cannot read\n", argv[2]); return 1; }
    fclose(fp);
    ivit_jpeg_desc desc;
    int64_t ncoef = 0;
    size_t plane_bytes = 0;
    st = ivit_jpeg_query_host(file, (size_t)file_bytes, &desc, &ncoef, &plane_bytes, msg, sizeof(msg));
    if (st != IVIT_OK) { fprintf(stderr, "classify_jpeg: %s: %s (%s)\n", argv[2], ivit_status_string(st), msg); return 1; }
    int16_t *coefs_host = (int16_t *)malloc((size_t)ncoef * sizeof(int16_t));
    if (!coefs_host) return 1;
    st = ivit_jpeg_entropy_decode_host(file, (size_t)file_bytes, coefs_host, ncoef, msg, sizeof(msg));
    if (st != IVIT_OK) { fprintf(stderr, "classify_jpeg: %s: %s (%s)\n", argv[2], ivit_status_string(st), msg); return 1; }
    const int crop = info.img_size, size = (int)(info.img_size / 0.875);

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
        IVIT(ivit_vit_workspace_bytes(vit, 1, 1, &ws_bytes));
    } else {
        IVIT(ivit_model_swin(m, &swin));
        IVIT(ivit_swin_workspace_bytes(swin, 1, 1, &ws_bytes));
    }

    /* one file: its coefficients, planes and pixels each start their buffer */
    const size_t pixels_bytes = (size_t)desc.w * desc.h * 3;
    const ivit_image_desc image = {0, desc.h, desc.w};
    size_t jpeg_ws_bytes = 0;
    IVIT(ivit_jpeg_workspace_bytes(&desc, 1, &jpeg_ws_bytes));
    int16_t *coefs = NULL;
    uint8_t *planes = NULL, *pixels = NULL;
    ivit_jpeg_desc *desc_dev = NULL;
    ivit_image_desc *image_dev = NULL;
    int8_t *input = NULL;
    void *ws = NULL;
    int32_t *logits = NULL, *idx = NULL;
    float *val = NULL;
    HIP(hipMalloc((void **)&coefs, (size_t)ncoef * sizeof(int16_t)));
    HIP(hipMalloc((void **)&planes, jpeg_ws_bytes));
    HIP(hipMalloc((void **)&pixels, pixels_bytes));
    HIP(hipMalloc((void **)&desc_dev, sizeof(desc)));
    HIP(hipMalloc((void **)&image_dev, sizeof(image)));
    HIP(hipMalloc((void **)&input, (size_t)3 * crop * crop));
    HIP(hipMalloc(&ws, ws_bytes ? ws_bytes : 1));
    HIP(hipMalloc((void **)&logits, (size_t)info.num_classes * 4));
    HIP(hipMalloc((void **)&idx, (size_t)k * 4));
    HIP(hipMalloc((void **)&val, (size_t)k * 4));
    HIP(hipMemcpy(coefs, coefs_host, (size_t)ncoef * sizeof(int16_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(desc_dev, &desc, sizeof(desc), hipMemcpyHostToDevice));
    HIP(hipMemcpy(image_dev, &image, sizeof(image), hipMemcpyHostToDevice));

    const float mean[3] = {0.485f, 0.456f, 0.406f}, std_[3] = {0.229f, 0.224f, 0.225f};
    IVIT(ivit_jpeg_reconstruct_u8(h, coefs, ncoef, &desc, desc_dev, 1, planes, jpeg_ws_bytes, pixels, pixels_bytes));
    IVIT(ivit_eval_transform_u8(h, pixels, pixels_bytes, &image, image_dev, 1, size, crop, mean, std_, info.s_input, input));
    if (vit) {
        IVIT(ivit_vit_workspace_init(vit, ws, ws_bytes, 1, 1));
        IVIT(ivit_vit_predict(vit, input, 1, 1, ws, ws_bytes, logits, (const float *)head_scale, k, idx, val));
    } else {
        IVIT(ivit_swin_predict(swin, input, 1, 1, ws, ws_bytes, logits, (const float *)head_scale, k, idx, val));
    }
    HIP(hipDeviceSynchronize());

    int32_t *idx_host = (int32_t *)malloc((size_t)k * 4);
    float *val_host = (float *)malloc((size_t)k * 4);
    if (!idx_host || !val_host) return 1;
    HIP(hipMemcpy(idx_host, idx, (size_t)k * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(val_host, val, (size_t)k * 4, hipMemcpyDeviceToHost));
    printf("0");
    for (int j = 0; j < k; ++j) printf(" %d:%.9g", idx_host[j], val_host[j]);
    printf("\n");

    free(idx_host); free(val_host); free(coefs_host); free(file);
    HIP(hipFree(val)); HIP(hipFree(idx)); HIP(hipFree(logits)); HIP(hipFree(ws)); HIP(hipFree(input)); HIP(hipFree(image_dev));
    HIP(hipFree(desc_dev)); HIP(hipFree(pixels)); HIP(hipFree(planes)); HIP(hipFree(coefs));
    IVIT(ivit_model_close(m));
    IVIT(ivit_destroy(h));
    return 0;
}
