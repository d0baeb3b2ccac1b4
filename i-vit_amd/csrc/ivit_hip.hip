// ivit_hip.hip — C-ABI (include/ivit.h, include/ivit_eval.h, include/ivit_features.h, include/ivit_attnmap.h, include/ivit_classmap.h,
// include/ivit_hidden.h, include/ivit_search.h, include/ivit_modelfile.h, include/ivit_probe.h, include/ivit_views.h, include/ivit_cluster.h, include/ivit_range.h, include/ivit_jpeg.h) over the gfx950
// kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// The launch idioms every entry point shares are defined once, below ivit_ctx: launch_dyn (the dynamic-LDS attribute, cached per
// device and kernel, then the launch), with_bool / with_width (one spelling of a launch for a pair of instantiations), and the
// range predicates rq_fast / rq_fast2 / attn_fast that choose instantiations and refuse calls.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <dlfcn.h>
#include <mutex>
#include <atomic>
#include <type_traits>
#include "ivit_device.h"
#include "ivit_elementwise.h"
#include "ivit_layernorm.h"
#include "ivit_gemm.h"
#include "ivit_attention.h"
#include "ivit_gemm2.h"
#include "ivit_gemm3.h"
#include "ivit_gemm_wreg.h"
#include "ivit_swin.h"
#include "ivit_mlp.h"
#include "ivit_mlp_rs.h"
#include "ivit_swin_mlp_rs.h"
#include "ivit_gemm_ws.h"
#include "ivit_swin12.h"
#include "ivit_topk.h"
#include "ivit_score.h"
#include "ivit_features.h"
#include "ivit_attnmap.h"
#include "ivit_classmap.h"
#include "ivit_hidden.h"
#include "ivit_search.h"
#include "ivit_probe.h"
#include "ivit_cluster.h"
#include "ivit_range.h"
#include "ivit_preprocess.h"
#include "ivit_views.h"
#include "ivit_jpeg_host.h"
#include "ivit_jpeg.h"

#define IVIT_MAX_DEVICES 64     // per-device caches of launch attributes (larger ordinals simply do not cache)
struct ivit_ctx {
    int device;
    hipStream_t stream;
    int num_cu;
    // CUs the one-workgroup-per-CU kernels (gemm_ws_qkv_kernel, mlp384rs_kernel / mlp384_kernel) size their grids for; 0 = num_cu.  The
    // whole-model runners give the handle of a slice stream its share of the device (num_cu / slices): a slice's launch then has the
    // per-workgroup geometry of the unsliced one (DeiT-S b256: one image per workgroup) and two slices' kernels run side by side on
    // disjoint CUs instead of as two half-filled grids of 256 (profiles/README.md, round 6, last session)
    int cu_share;
    char err[256];
};
static inline int persistent_cus(const ivit_ctx *h) { return h->cu_share > 0 ? h->cu_share : h->num_cu; }

// every entry point binds the calling thread to the handle's device for the duration of the call and puts the caller's
// current device back on the way out: one process may drive several GPUs through several handles, and a torch (or any
// other HIP) user of the same thread keeps allocating / launching where it was
struct ivit_device_guard {
    int prev = -1;
    bool restore = false;
    bool enter(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == dev) return true;
        if (hipSetDevice(dev) != hipSuccess) return false;
        restore = prev >= 0;
        return true;
    }
    ~ivit_device_guard() { if (restore) (void)hipSetDevice(prev); }
};
#define CHECK_H(h) if (!(h)) return IVIT_ERR_INVALID; ivit_device_guard ivit_dev_guard_; if (!ivit_dev_guard_.enter((h)->device)) return IVIT_ERR_HIP
#define REQUIRE(h, cond, msg) do { if (!(cond)) { snprintf((h)->err, sizeof((h)->err), "%s: %s", __func__, msg); return IVIT_ERR_INVALID; } } while (0)
// An activation or output pointer that a kernel touches through vector accesses wider than its element (include/ivit.h, Conventions):
// refused unless aligned to that width, before anything is launched.  `name` is the argument as the header spells it.
#define REQUIRE_ALIGNED(h, p, name, bytes) REQUIRE(h, ((uintptr_t)(p) & ((bytes) - 1)) == 0, name " must be " #bytes "-byte aligned")
#define REQUIRE_A16(h, p, name) REQUIRE_ALIGNED(h, p, name, 16)
// Overlapping arguments (include/ivit.h, Conventions): an array an entry writes may overlap neither an activation array it reads nor
// another array it writes; judged on the byte extents [p, p + bytes) the header documents, refused before anything is launched.  Host
// pointer comparisons only.  ranges_disjoint takes the two ranges, the two argument names as the header spells them and the message
// (what the arrays are to the entry); a null pointer or an empty range overlaps nothing.
static inline bool ranges_disjoint(ivit_ctx *h, const char *fn, const void *a, size_t a_bytes, const char *a_name, const void *b, size_t b_bytes,
                                   const char *b_name, const char *msg) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    if (!a || !b || !a_bytes || !b_bytes || a0 + a_bytes <= b0 || b0 + b_bytes <= a0) return true;
    snprintf(h->err, sizeof(h->err), "%s: %s and %s overlap: %s", fn, a_name, b_name, msg);
    return false;
}
#define REQUIRE_DISJOINT(h, a, a_bytes, a_name, b, b_bytes, b_name, msg) \
    do { if (!ranges_disjoint(h, __func__, a, (size_t)(a_bytes), a_name, b, (size_t)(b_bytes), b_name, msg)) return IVIT_ERR_INVALID; } while (0)
// an in-place pair (the entry's "Overlap:" line names it): the same pointer with the same extent is accepted, every other overlap refused
#define REQUIRE_DISJOINT_OR_SAME(h, a, a_bytes, a_name, b, b_bytes, b_name, msg) \
    do { if (!((const void *)(a) == (const void *)(b) && (size_t)(a_bytes) == (size_t)(b_bytes)) && \
             !ranges_disjoint(h, __func__, a, (size_t)(a_bytes), a_name, b, (size_t)(b_bytes), b_name, msg)) return IVIT_ERR_INVALID; } while (0)
// bytes spanned by `rows` rows of `payload` elements at a pitch of `pitch` elements, `elem` bytes each: (rows - 1) * pitch + payload
static inline size_t span_bytes(long long rows, long long pitch, long long payload, size_t elem) {
    return rows > 0 ? (size_t)((rows - 1) * pitch + payload) * elem : 0;
}
#define OVL_IN "an output may not overlap an activation input"
#define OVL_OUT "two arrays the entry writes may not overlap"
// the qkv scatter's arrays (ivit_linear_i8_qkv and its planned / LayerNorm-headed forms): the input against q, k and v, and the three
// among themselves; q and k are [B*H, T, dh], v the same at ldv == 0 and B*H*dh rows of T at a pitch of ldv otherwise.  `fn`: the entry
static int qkv_disjoint(ivit_ctx *h, const char *fn, const void *x, size_t x_bytes, const char *x_name, const int8_t *q, const int8_t *k,
                        const int8_t *vt, int B, int T, int H, int dh, int ldv) {
    const size_t nqk = (size_t)B * H * T * dh, nv = ldv == 0 ? nqk : span_bytes((long long)B * H * dh, ldv, T, 1);
    const bool ok = ranges_disjoint(h, fn, x, x_bytes, x_name, q, nqk, "q", OVL_IN) && ranges_disjoint(h, fn, x, x_bytes, x_name, k, nqk, "k", OVL_IN) &&
                    ranges_disjoint(h, fn, x, x_bytes, x_name, vt, nv, "vt", OVL_IN) && ranges_disjoint(h, fn, q, nqk, "q", k, nqk, "k", OVL_OUT) &&
                    ranges_disjoint(h, fn, q, nqk, "q", vt, nv, "vt", OVL_OUT) && ranges_disjoint(h, fn, k, nqk, "k", vt, nv, "vt", OVL_OUT);
    return ok ? IVIT_OK : IVIT_ERR_INVALID;
}
// the batched NT products: batch b of an operand spans (rows - 1) * ld + payload elements from b * stride (strides in elements, A's
// elements a_elem bytes wide, C's four); a negative stride is outside what the extents describe and is not judged
static int bmm_disjoint(ivit_ctx *h, const char *fn, const void *A, size_t a_elem, const int8_t *B, const int32_t *C, int nb, int M, int N, int K,
                        int lda, int ldb, int ldc, long long strideA, long long strideB, long long strideC) {
    if (strideA < 0 || strideB < 0 || strideC < 0 || lda < 0 || ldb < 0 || ldc < 0) return IVIT_OK;
    const size_t nA = ((size_t)(nb - 1) * strideA + span_bytes(M, lda, K, 1)) * a_elem, nB = (size_t)(nb - 1) * strideB + span_bytes(N, ldb, K, 1);
    const size_t nC = ((size_t)(nb - 1) * strideC + span_bytes(M, ldc, N, 1)) * 4;
    return ranges_disjoint(h, fn, A, nA, "A", C, nC, "C", OVL_IN) && ranges_disjoint(h, fn, B, nB, "B", C, nC, "C", OVL_IN) ? IVIT_OK : IVIT_ERR_INVALID;
}
#define LAUNCH_CHECK(h) do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { snprintf((h)->err, sizeof((h)->err), "%s: %s", __func__, hipGetErrorString(e_)); return IVIT_ERR_HIP; } } while (0)

// A launch's global size (blocks x threads) must stay below 2^32: the runtime takes a larger one modulo 2^32 and runs the remainder
// without an error, so the rows behind it are never written.  An entry whose grid grows with the caller's row count refuses such a
// call before anything is launched (include/ivit.h, Conventions); `per_block`: rows (images, elements) a block works, for the message
static inline int launch_fits(ivit_ctx *h, const char *fn, long long blocks, int threads, long long per_block) {
    if (blocks * threads < (1LL << 32)) return IVIT_OK;
    snprintf(h->err, sizeof(h->err), "%s: %lld blocks of %d threads are 2^32 work-items or more: one call takes at most %lld rows", fn, blocks, threads,
             ((1LL << 32) / threads - 1) * per_block);
    return IVIT_ERR_UNSUPPORTED;
}
#define REQUIRE_LAUNCH(h, blocks, threads, per_block) do { if (int st_ = launch_fits(h, __func__, blocks, threads, per_block)) return st_; } while (0)

// Launch `Kernel` with `lds` bytes of dynamic LDS.  Above 64 KB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize: set once
// per device and kernel for the largest size seen (the attribute is a maximum), so the eager single-stream modes pay no host call
// per launch; a device ordinal outside the cache sets it every time.  Per DEVICE: ADVICE r5, one process-wide flag left the second
// GPU of a process without it.  Returns the attribute's status; the caller checks the launch itself (LAUNCH_CHECK).
template <auto Kernel, class... Args>
static int launch_dyn(ivit_handle h, dim3 grid, dim3 block, size_t lds, const Args &...args) {
    if (lds > 65536) {
        static std::atomic<int> max_dev[IVIT_MAX_DEVICES];
        const bool cached = h->device >= 0 && h->device < IVIT_MAX_DEVICES;
        if (!cached || max_dev[h->device].load(std::memory_order_acquire) < (int)lds) {
            hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "hipFuncSetAttribute: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
            if (cached) max_dev[h->device].store((int)lds, std::memory_order_release);
        }
    }
    Kernel<<<grid, block, lds, h->stream>>>(args...);
    return IVIT_OK;
}

// f(std::true_type) or f(std::false_type): a launch site names a <bool FMA> (or <bool LN>) kernel pair once
template <class F>
static inline auto with_bool(bool on, F &&f) {
    if (on) return f(std::true_type{});
    return f(std::false_type{});
}
// the same for the two stage-0 widths of the token-order LayerNorm
template <class F>
static inline auto with_width(int C, F &&f) {
    if (C == 96) return f(std::integral_constant<int, 96>{});
    return f(std::integral_constant<int, 128>{});
}

// The range predicates: they choose which instantiation runs and which calls are refused, so each has ONE definition.
// rq_fast: |m * 2^-e| below RQ_FAST_CLIM (ivit_device.h), where a 16-bit value times the multiplier is exact in the kernels' fast
// requant.  attn_fast: both attention multipliers inside (-512, 512), the bound of attn_fused_kernel<FAST = true>.  It was
// spelled `c < 512 && c > -512` at some sites and `fabs(c) < 512` at others: the two agree on every input, NaN included (every
// comparison with a NaN is false, and fabs(NaN) is a NaN)
static inline bool rq_fast(ivit_dyadic d) { return fabs(d.m * d.r) < RQ_FAST_CLIM; }
static inline bool rq_fast2(ivit_dyadic a, ivit_dyadic b) { return rq_fast(a) && rq_fast(b); }
static inline bool attn_fast(ivit_dyadic dy_qk, ivit_dyadic dy_pv) { return fabs(dy_qk.m * dy_qk.r) < 512.0 && fabs(dy_pv.m * dy_pv.r) < 512.0; }

extern "C" {

int ivit_version(void) { return IVIT_VERSION; }

const char *ivit_status_string(int s) {
    switch (s) {
        case IVIT_OK: return "ok";
        case IVIT_ERR_INVALID: return "invalid argument";
        case IVIT_ERR_HIP: return "HIP runtime error";
        case IVIT_ERR_UNSUPPORTED: return "unsupported shape";
        case IVIT_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

int ivit_create(ivit_handle *out, int device, void *hip_stream) {
    if (!out) return IVIT_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return IVIT_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return IVIT_ERR_HIP;
    ivit_ctx *c = new (std::nothrow) ivit_ctx();
    if (!c) return IVIT_ERR_HIP;
    c->device = device;
    c->stream = (hipStream_t)hip_stream;
    c->err[0] = 0;
    c->cu_share = 0;
    hipDeviceProp_t prop;
    c->num_cu = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 256;
    *out = c;
    return IVIT_OK;
}

int ivit_destroy(ivit_handle h) {
    CHECK_H(h);
    delete h;
    return IVIT_OK;
}

int ivit_set_stream(ivit_handle h, void *hip_stream) {
    CHECK_H(h);
    h->stream = (hipStream_t)hip_stream;
    return IVIT_OK;
}

int ivit_set_cu_share(ivit_handle h, int cus) {
    CHECK_H(h);
    REQUIRE(h, cus >= 0, "cus must be >= 0 (0 = the whole device)");
    h->cu_share = cus > h->num_cu ? h->num_cu : cus;
    return IVIT_OK;
}

const char *ivit_last_error(ivit_handle h) { return h ? h->err : "null handle"; }

static inline int grid_for(ivit_handle h, long long work_items, int per_block) {
    long long g = (work_items + per_block - 1) / per_block;
    long long cap = (long long)h->num_cu * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

int ivit_quantize_input_f32(ivit_handle h, const float *x, float scale, int8_t *q, int64_t n) {
    CHECK_H(h);
    REQUIRE(h, x && q && n >= 0 && scale > 0.f, "bad arguments");
    REQUIRE_A16(h, x, "x");                 // four floats per load, four packed bytes per store
    REQUIRE_ALIGNED(h, q, "q", 4);
    REQUIRE_DISJOINT(h, x, (size_t)n * 4, "x", q, (size_t)n, "q", OVL_IN);
    if (n == 0) return IVIT_OK;
    quantize_input_kernel<<<grid_for(h, n, 1024), 256, 0, h->stream>>>(x, scale, q, n);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_resize_center_crop_u8(ivit_handle h, const uint8_t *hwc, int B, int H0, int W0, int size, int crop,
                               float *workspace, uint8_t *out_hwc) {
    CHECK_H(h);
    REQUIRE(h, hwc && workspace && out_hwc && B > 0 && H0 > 0 && W0 > 0 && size > 0 && crop > 0, "bad arguments");
    // torchvision Resize(int): the SHORTER side becomes `size`, the longer int(size * long / short); CenterCrop offsets
    // int(round((dim - crop) / 2.0))
    int Hr, Wr;
    if (H0 <= W0) { Hr = size; Wr = (int)((long long)size * W0 / H0); }
    else { Wr = size; Hr = (int)((long long)size * H0 / W0); }
    REQUIRE(h, crop <= Hr && crop <= Wr, "crop larger than the resized image");
    {
        const size_t nin = (size_t)B * H0 * W0 * 3, nws = (size_t)B * H0 * crop * 3 * sizeof(float), nout = (size_t)B * crop * crop * 3;
        REQUIRE_DISJOINT(h, hwc, nin, "hwc", workspace, nws, "workspace", OVL_IN);
        REQUIRE_DISJOINT(h, hwc, nin, "hwc", out_hwc, nout, "out_hwc", OVL_IN);
        REQUIRE_DISJOINT(h, workspace, nws, "workspace", out_hwc, nout, "out_hwc", OVL_OUT);
    }
    const int top = (int)__builtin_rint((Hr - crop) / 2.0), left = (int)__builtin_rint((Wr - crop) / 2.0);
    resize_h_kernel<<<grid_for(h, (long long)B * H0 * crop, 256), 256, 0, h->stream>>>(hwc, B, H0, W0, Wr, left, crop, workspace);
    resize_v_kernel<<<grid_for(h, (long long)B * crop * crop, 256), 256, 0, h->stream>>>(workspace, B, H0, Hr, top, crop, out_hwc);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_normalize_quantize_u8(ivit_handle h, const uint8_t *hwc, int B, int H, int W, const float mean[3],
                               const float std_[3], float scale, int8_t *nchw) {
    CHECK_H(h);
    REQUIRE(h, hwc && nchw && mean && std_ && B > 0 && H > 0 && W > 0 && scale > 0.f, "bad arguments");
    REQUIRE(h, std_[0] != 0.f && std_[1] != 0.f && std_[2] != 0.f, "zero std");
    REQUIRE_DISJOINT(h, hwc, (size_t)B * H * W * 3, "hwc", nchw, (size_t)B * H * W * 3, "nchw", OVL_IN);
    normalize_quantize_u8_kernel<<<grid_for(h, (long long)B * H * W, 256), 256, 0, h->stream>>>(
        hwc, B, H, W, mean[0], mean[1], mean[2], std_[0], std_[1], std_[2], scale, nchw);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the PIL-pinned ragged front end (ivit_preprocess.h)
// The checks of the host descriptor table, then ONE launch over the device table: ceil(crop / PIL_BAND) x B workgroups, a function of
// B and crop only.  `fn` names the entry in ivit_last_error.
template <bool NCHW>
static int launch_pil_eval(ivit_handle h, const char *fn, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *desc_host,
                           const ivit_image_desc *desc_dev, int B, int size, int crop, const float *mean, const float *std_, float scale,
                           void *out) {
    auto fail = [&](const char *msg, int i) {
        if (i >= 0) snprintf(h->err, sizeof(h->err), "%s: image %d: %s", fn, i, msg);
        else snprintf(h->err, sizeof(h->err), "%s: %s", fn, msg);
        return IVIT_ERR_INVALID;
    };
    if (!(pixels && desc_host && desc_dev && out && B > 0 && size > 0 && crop > 0)) return fail("bad arguments", -1);
    if (NCHW) {
        if (!(mean && std_ && scale > 0.f)) return fail("bad arguments", -1);
        if (!(std_[0] != 0.f && std_[1] != 0.f && std_[2] != 0.f)) return fail("zero std", -1);
    }
    const int nbands = (crop + PIL_BAND - 1) / PIL_BAND;
    if ((long long)nbands * B * PIL_THREADS >= (1LL << 32)) return fail("B * ceil(crop / 32) blocks of 512 threads are 2^32 work-items or more", -1);
    {   // the output against the whole pixel blob [pixels, pixels + pixels_bytes) and the device descriptor table
        const size_t nout = (size_t)B * crop * crop * 3;
        const char *oname = NCHW ? "nchw" : "out_hwc";
        if (!ranges_disjoint(h, fn, pixels, pixels_bytes, "pixels", out, nout, oname, OVL_IN) ||
            !ranges_disjoint(h, fn, desc_dev, (size_t)B * sizeof(ivit_image_desc), "desc_dev", out, nout, oname, OVL_IN))
            return IVIT_ERR_INVALID;
    }
    for (int i = 0; i < B; ++i) {
        const ivit_image_desc &d = desc_host[i];
        if (d.h <= 0 || d.w <= 0) return fail("non-positive side", i);
        if (d.offset < 0) return fail("negative offset", i);
        const unsigned __int128 end = (unsigned __int128)d.offset + (unsigned __int128)d.h * (unsigned __int128)d.w * 3u;
        if (end > (unsigned __int128)pixels_bytes) return fail("reaches past pixels_bytes", i);
        long long Hr, Wr;                  // torchvision Resize(int), as in ivit_resize_center_crop_u8 and pil_eval_kernel
        if (d.h <= d.w) { Hr = size; Wr = (long long)size * d.w / d.h; }
        else { Wr = size; Hr = (long long)size * d.h / d.w; }
        if (crop > Hr || crop > Wr) return fail("crop larger than the resized image", i);
    }
    const float z = 0.f;
    const int st = launch_dyn<pil_eval_kernel<NCHW>>(h, dim3((unsigned)(nbands * B)), dim3(PIL_THREADS), (size_t)PIL_LDS_BYTES,
                                                      (const unsigned char *)pixels, desc_dev, size, crop, nbands, NCHW ? mean[0] : z,
                                                      NCHW ? mean[1] : z, NCHW ? mean[2] : z, NCHW ? std_[0] : z, NCHW ? std_[1] : z,
                                                      NCHW ? std_[2] : z, NCHW ? scale : z, (unsigned char *)out);
    if (st != IVIT_OK) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" {

int ivit_resize_center_crop_u8_pil(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *desc_host,
                                   const ivit_image_desc *desc_dev, int B, int size, int crop, uint8_t *out_hwc) {
    CHECK_H(h);
    return launch_pil_eval<false>(h, __func__, pixels, pixels_bytes, desc_host, desc_dev, B, size, crop, nullptr, nullptr, 0.f, out_hwc);
}

int ivit_eval_transform_u8(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *desc_host,
                           const ivit_image_desc *desc_dev, int B, int size, int crop, const float mean[3], const float std_[3],
                           float scale, int8_t *nchw) {
    CHECK_H(h);
    return launch_pil_eval<true>(h, __func__, pixels, pixels_bytes, desc_host, desc_dev, B, size, crop, mean, std_, scale, nchw);
}

}  // extern "C"

// ---------------------------------------------------------------- image views (include/ivit_views.h, ivit_views.h)
// The checks of both host tables, then ONE launch over the device tables: ceil(crop / PIL_BAND) x V workgroups.  What the checks
// establish is what keeps the kernel inside pixels_bytes: every image inside the blob, every box inside its image (the taps of a view
// stay inside its box), every window inside the resized box.
template <bool NCHW>
static int launch_pil_views(ivit_handle h, const char *fn, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *img_host,
                            const ivit_image_desc *img_dev, int B, const ivit_view_desc *view_host, const ivit_view_desc *view_dev, int V,
                            int crop, const float *mean, const float *std_, float scale, void *out) {
    auto fail = [&](const char *what, const char *msg, int i) {
        if (i >= 0) snprintf(h->err, sizeof(h->err), "%s: %s %d: %s", fn, what, i, msg);
        else snprintf(h->err, sizeof(h->err), "%s: %s", fn, msg);
        return IVIT_ERR_INVALID;
    };
    if (!(pixels && img_host && img_dev && out && B > 0 && V >= 0 && crop > 0 && (V == 0 || (view_host && view_dev))))
        return fail("", "bad arguments", -1);
    if (NCHW) {
        if (!(mean && std_ && scale > 0.f)) return fail("", "bad arguments", -1);
        if (!(std_[0] != 0.f && std_[1] != 0.f && std_[2] != 0.f)) return fail("", "zero std", -1);
    }
    const int nbands = (crop + PIL_BAND - 1) / PIL_BAND;
    if ((long long)nbands * V * PIL_THREADS >= (1LL << 32)) return fail("", "V * ceil(crop / 32) blocks of 512 threads are 2^32 work-items or more", -1);
    {   // the output against the whole pixel blob and both device tables
        const size_t nout = (size_t)V * crop * crop * 3;
        const char *oname = NCHW ? "nchw" : "out_hwc";
        if (!ranges_disjoint(h, fn, pixels, pixels_bytes, "pixels", out, nout, oname, OVL_IN) ||
            !ranges_disjoint(h, fn, img_dev, (size_t)B * sizeof(ivit_image_desc), "img_dev", out, nout, oname, OVL_IN) ||
            !ranges_disjoint(h, fn, view_dev, (size_t)V * sizeof(ivit_view_desc), "view_dev", out, nout, oname, OVL_IN))
            return IVIT_ERR_INVALID;
    }
    for (int i = 0; i < B; ++i) {
        const ivit_image_desc &d = img_host[i];
        if (d.h <= 0 || d.w <= 0) return fail("image", "non-positive side", i);
        if (d.offset < 0) return fail("image", "negative offset", i);
        const unsigned __int128 end = (unsigned __int128)d.offset + (unsigned __int128)d.h * (unsigned __int128)d.w * 3u;
        if (end > (unsigned __int128)pixels_bytes) return fail("image", "reaches past pixels_bytes", i);
    }
    for (int i = 0; i < V; ++i) {
        const ivit_view_desc &v = view_host[i];
        if (v.image < 0 || v.image >= B) return fail("view", "image outside the image table", i);
        const ivit_image_desc &d = img_host[v.image];
        if (v.bw < 1 || v.bh < 1) return fail("view", "empty box", i);
        if (v.x0 < 0 || v.y0 < 0 || (long long)v.x0 + v.bw > d.w || (long long)v.y0 + v.bh > d.h) return fail("view", "box outside the image", i);
        if (v.rw < 1 || v.rh < 1 || v.rw > 65536 || v.rh > 65536) return fail("view", "resized size outside 1 .. 65536", i);
        if (v.left < 0 || v.top < 0 || (long long)v.left + crop > v.rw || (long long)v.top + crop > v.rh)
            return fail("view", "window outside the resized box", i);
        if (v.flip != 0 && v.flip != 1) return fail("view", "flip must be 0 or 1", i);
    }
    if (V == 0) return IVIT_OK;
    const float z = 0.f;
    const int st = launch_dyn<pil_view_kernel<NCHW>>(h, dim3((unsigned)(nbands * V)), dim3(PIL_THREADS), (size_t)PIL_LDS_BYTES,
                                                      (const unsigned char *)pixels, img_dev, view_dev, crop, nbands, NCHW ? mean[0] : z,
                                                      NCHW ? mean[1] : z, NCHW ? mean[2] : z, NCHW ? std_[0] : z, NCHW ? std_[1] : z,
                                                      NCHW ? std_[2] : z, NCHW ? scale : z, (unsigned char *)out);
    if (st != IVIT_OK) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" {

int ivit_view_resize_u8_pil(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *img_host,
                            const ivit_image_desc *img_dev, int B, const ivit_view_desc *view_host, const ivit_view_desc *view_dev, int V,
                            int crop, uint8_t *out_hwc) {
    CHECK_H(h);
    return launch_pil_views<false>(h, __func__, pixels, pixels_bytes, img_host, img_dev, B, view_host, view_dev, V, crop, nullptr, nullptr,
                                   0.f, out_hwc);
}

int ivit_view_transform_u8(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *img_host,
                           const ivit_image_desc *img_dev, int B, const ivit_view_desc *view_host, const ivit_view_desc *view_dev, int V,
                           int crop, const float mean[3], const float std_[3], float scale, int8_t *nchw) {
    CHECK_H(h);
    return launch_pil_views<true>(h, __func__, pixels, pixels_bytes, img_host, img_dev, B, view_host, view_dev, V, crop, mean, std_, scale,
                                  nchw);
}

int ivit_logits_view_sum(ivit_handle h, const int32_t *logits, int groups, int views, int num_classes, int32_t *out) {
    CHECK_H(h);
    REQUIRE(h, logits && out && groups >= 0 && num_classes >= 1, "bad arguments");
    REQUIRE(h, views >= 1 && views <= VIEW_SUM_MAX_VIEWS, "views must be in 1 .. 64");
    REQUIRE_DISJOINT(h, logits, (size_t)groups * views * num_classes * 4, "logits", out, (size_t)groups * num_classes * 4, "out", OVL_IN);
    if (groups == 0) return IVIT_OK;
    const bool vec = num_classes % 4 == 0 && (((uintptr_t)logits | (uintptr_t)out) & 15) == 0;
    const long long per = vec ? num_classes / 4 : num_classes, n = (long long)groups * per;
    const int grid = grid_for(h, n, VIEW_SUM_THREADS);              // a grid-stride stream: at most 16 blocks per CU
    if (vec) logits_view_sum_kernel<true><<<grid, VIEW_SUM_THREADS, 0, h->stream>>>(logits, n, per, views, out);
    else logits_view_sum_kernel<false><<<grid, VIEW_SUM_THREADS, 0, h->stream>>>(logits, n, per, views, out);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- JPEG input (include/ivit_jpeg.h, ivit_jpeg_host.h, ivit_jpeg.h)
// The two host entries are ivit_jpeg_host.h's functions.  The reconstruction checks the host table — what keeps both kernels inside
// coef_count, workspace_bytes and pixels_bytes: every grid recomputed from (w, h, hs, vs), every range inside its buffer, the written
// ranges ascending — then two launches over the device table, gridDim.y the file, gridDim.x sized for the largest file.
static inline size_t jpeg_align16(size_t n) { return (n + 15) & ~(size_t)15; }

extern "C" {

int ivit_jpeg_query_host(const uint8_t *data_host, size_t bytes, ivit_jpeg_desc *desc_host, int64_t *coef_count, size_t *workspace_bytes,
                         char *err_host, size_t err_bytes) {
    return ivit_jpeg_host_query(data_host, bytes, desc_host, coef_count, workspace_bytes, err_host, err_bytes);
}

int ivit_jpeg_entropy_decode_host(const uint8_t *data_host, size_t bytes, int16_t *coefs_host, int64_t coef_capacity, char *err_host,
                                  size_t err_bytes) {
    return ivit_jpeg_host_entropy_decode(data_host, bytes, coefs_host, coef_capacity, err_host, err_bytes);
}

int ivit_jpeg_workspace_bytes(const ivit_jpeg_desc *desc_host, int B, size_t *bytes) {
    if (!bytes || B < 0 || (B > 0 && !desc_host)) return IVIT_ERR_INVALID;
    size_t n = 0;
    for (int i = 0; i < B; ++i) {
        const ivit_jpeg_desc &d = desc_host[i];
        if (d.ncomp != 1 && d.ncomp != 3) return IVIT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (d.bw[c] < 0 || d.bh[c] < 0 || d.bw[c] > 8192 || d.bh[c] > 8192) return IVIT_ERR_INVALID;
        n += jpeg_align16(ivit_jpeg_host::plane_bytes(d.bw, d.bh, d.ncomp));
    }
    *bytes = n;
    return IVIT_OK;
}

int ivit_jpeg_reconstruct_u8(ivit_handle h, const int16_t *coefs, int64_t coef_count, const ivit_jpeg_desc *desc_host,
                             const ivit_jpeg_desc *desc_dev, int B, uint8_t *workspace, size_t workspace_bytes, uint8_t *pixels,
                             size_t pixels_bytes) {
    CHECK_H(h);
    REQUIRE(h, B >= 0 && coef_count >= 0, "bad arguments");
    if (B == 0) return IVIT_OK;
    REQUIRE(h, coefs && desc_host && desc_dev && workspace && pixels, "bad arguments");
    REQUIRE_A16(h, coefs, "coefs");
    REQUIRE_A16(h, workspace, "workspace");
    REQUIRE_ALIGNED(h, desc_dev, "desc_dev", 8);
    const size_t ncoef = (size_t)coef_count * 2, ndesc = (size_t)B * sizeof(ivit_jpeg_desc);
    REQUIRE_DISJOINT(h, pixels, pixels_bytes, "pixels", workspace, workspace_bytes, "workspace", OVL_OUT);
    REQUIRE_DISJOINT(h, coefs, ncoef, "coefs", pixels, pixels_bytes, "pixels", OVL_IN);
    REQUIRE_DISJOINT(h, desc_dev, ndesc, "desc_dev", pixels, pixels_bytes, "pixels", OVL_IN);
    REQUIRE_DISJOINT(h, coefs, ncoef, "coefs", workspace, workspace_bytes, "workspace", OVL_IN);
    REQUIRE_DISJOINT(h, desc_dev, ndesc, "desc_dev", workspace, workspace_bytes, "workspace", OVL_IN);
    auto fail = [&](const char *msg, int i) {
        snprintf(h->err, sizeof(h->err), "%s: image %d: %s", __func__, i, msg);
        return IVIT_ERR_INVALID;
    };
    long long max_blocks = 0, max_pixels = 0;
    unsigned __int128 pixel_end = 0, plane_end = 0;
    for (int i = 0; i < B; ++i) {
        const ivit_jpeg_desc &d = desc_host[i];
        if (d.w < 1 || d.h < 1 || d.w > 65535 || d.h > 65535) return fail("side outside 1 .. 65535", i);
        if (d.ncomp != 1 && d.ncomp != 3) return fail("ncomp must be 1 or 3", i);
        const bool samp = (d.hs == 1 && d.vs == 1) || (d.ncomp == 3 && d.hs == 2 && (d.vs == 1 || d.vs == 2));
        if (!samp) return fail("sampling must be 1x1, 2x1 or 2x2 (1x1 with one component)", i);
        if (d.reserved != 0) return fail("reserved must be 0", i);
        const int mw = (d.w + 8 * d.hs - 1) / (8 * d.hs), mh = (d.h + 8 * d.vs - 1) / (8 * d.vs);
        long long blocks = 0;
        for (int c = 0; c < 3; ++c) {
            const int bw = c < d.ncomp ? mw * (c == 0 ? d.hs : 1) : 0, bh = c < d.ncomp ? mh * (c == 0 ? d.vs : 1) : 0;
            if (d.bw[c] != bw || d.bh[c] != bh) return fail("bw / bh are not the block grid of w, h and the sampling", i);
            blocks += (long long)bw * bh;
        }
        if (d.coef_offset < 0 || (d.coef_offset & 7)) return fail("coef_offset must be a non-negative multiple of 8", i);
        if ((unsigned __int128)d.coef_offset + (unsigned __int128)blocks * 64 > (unsigned __int128)coef_count) return fail("coefficients reach past coef_count", i);
        if (d.plane_offset < 0 || (d.plane_offset & 15)) return fail("plane_offset must be a non-negative multiple of 16", i);
        if ((unsigned __int128)d.plane_offset + (unsigned __int128)blocks * 64 > (unsigned __int128)workspace_bytes) return fail("planes reach past workspace_bytes", i);
        if (d.pixel_offset < 0) return fail("negative pixel_offset", i);
        const long long npix = (long long)d.w * d.h;
        if ((unsigned __int128)d.pixel_offset + (unsigned __int128)npix * 3 > (unsigned __int128)pixels_bytes) return fail("pixels reach past pixels_bytes", i);
        if ((unsigned __int128)d.pixel_offset < pixel_end) return fail("pixel_offset inside an earlier image's pixels", i);
        if ((unsigned __int128)d.plane_offset < plane_end) return fail("plane_offset inside an earlier image's planes", i);
        pixel_end = (unsigned __int128)d.pixel_offset + (unsigned __int128)npix * 3;
        plane_end = (unsigned __int128)d.plane_offset + (unsigned __int128)blocks * 64;
        max_blocks = std::max(max_blocks, blocks);
        max_pixels = std::max(max_pixels, npix);
    }
    REQUIRE(h, B <= 65535, "one call takes at most 65535 images");
    const long long g1 = (max_blocks + JPEG_WG_BLOCKS - 1) / JPEG_WG_BLOCKS, g2 = (max_pixels + JPEG_THREADS - 1) / JPEG_THREADS;
    REQUIRE_LAUNCH(h, g1 * B, JPEG_THREADS, 1);
    REQUIRE_LAUNCH(h, g2 * B, JPEG_THREADS, 1);
    jpeg_idct_kernel<<<dim3((unsigned)g1, (unsigned)B), JPEG_THREADS, 0, h->stream>>>((const short *)coefs, desc_dev, workspace);
    LAUNCH_CHECK(h);
    jpeg_color_kernel<<<dim3((unsigned)g2, (unsigned)B), JPEG_THREADS, 0, h->stream>>>(workspace, desc_dev, pixels);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- GEMM launchers
template <bool A16, int EPI>
static int launch_gemm(ivit_handle h, GemmArgs &a, int nb) {
    // the matrices of a batched product are gridDim.y: more than 65535 of them are refused here, before the launch would fail
    if (nb > 65535) {
        snprintf(h->err, sizeof(h->err), "batched product of %d matrices: one launch takes at most 65535 (nb, BH, B * H <= 65535)", nb);
        return IVIT_ERR_UNSUPPORTED;
    }
    const int tm = (a.M + GEMM_BM - 1) / GEMM_BM;
    a.tiles_n = (a.N + GEMM_BN - 1) / GEMM_BN;
    dim3 grid((unsigned)(tm * a.tiles_n), (unsigned)nb, 1);
    gemm_nt_kernel<A16, EPI><<<grid, 256, 0, h->stream>>>(a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// production path for the QuantLinear GEMMs: K % 64 == 0, int8 A, requant epilogues
template <int EPI>
static int launch_gemm2(ivit_handle h, GemmArgs &a) {
    a.tiles_n = (a.N + G2_BN - 1) / G2_BN;
    // tile height: estimated time ~ ceil(tiles / resident slots) * rows per tile; 256-row tiles run
    // 2 per CU, 128-row tiles 3 per CU.  Ties go to the larger tile (better operand reuse).
    const long long t256 = (long long)((a.M + 255) / 256) * a.tiles_n, t128 = (long long)((a.M + 127) / 128) * a.tiles_n;
    const long long s256 = 2LL * h->num_cu, s128 = (G2_NSTAGE128 == 2 ? 4LL : 3LL) * h->num_cu;
    const long long c256 = ((t256 + s256 - 1) / s256) * 256, c128 = ((t128 + s128 - 1) / s128) * 128;
    if (c128 < c256) gemm_glds_kernel<EPI, 128><<<dim3((unsigned)t128), 256, 0, h->stream>>>(a);
    else gemm_glds_kernel<EPI, 256><<<dim3((unsigned)t256), 512, 0, h->stream>>>(a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}
static inline bool use_gemm2(const GemmArgs &a) { return (a.K % 32) == 0 && a.K >= 64 && (a.lda % 16) == 0 && (a.ldb % 16) == 0; }

// short-K streaming kernel (ivit_gemm_wreg.h): K = 96 / 128 / 192 with whole 32-channel tiles in groups of 3 or 2, plain row-major
// operands, enough rows to keep every CU busy
static inline int wreg_nct(const GemmArgs &a) {
    if (a.K % 32 || !(a.K == 96 || a.K == 128 || a.K == 192) || a.N % 32 || a.lda != a.K || a.ldb != a.K ||
        a.ldc != a.N || a.M < 8192 || a.inner != 1)
        return 0;
    const int nt = a.N / 32;
    return nt % 3 == 0 ? 3 : (nt % 2 == 0 ? 2 : 0);
}
template <int EPI, int KS, int NCT>
static int launch_wreg_k(ivit_handle h, const GemmArgs &a) {
    const int ncg = a.N / (32 * NCT);
    // resident workgroups per CU of this instantiation (registers, LDS): asked once PER DEVICE (a process-wide
    // static reused the first device's answer on every other one); a race between host threads stores the same value twice
    static std::atomic<int> wpc_dev[IVIT_MAX_DEVICES];
    const bool cached = h->device >= 0 && h->device < IVIT_MAX_DEVICES;
    int wpc = cached ? wpc_dev[h->device].load(std::memory_order_relaxed) : 0;
    if (!wpc) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gemm_wreg_kernel<EPI, KS, NCT>, GW_THREADS, 0) != hipSuccess || n < 1) n = 1;
        wpc = n;
        if (cached) wpc_dev[h->device].store(n, std::memory_order_relaxed);
    }
    int per = (h->num_cu * wpc) / (8 * ncg);
    if (per < 1) per = 1;
    gemm_wreg_kernel<EPI, KS, NCT><<<dim3((unsigned)(8 * ncg * per)), GW_THREADS, 0, h->stream>>>(a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}
template <int EPI>
static int launch_wreg(ivit_handle h, const GemmArgs &a, int nct) {
    const int ks = a.K / 32;
    if (nct == 3) return ks == 3 ? launch_wreg_k<EPI, 3, 3>(h, a) : (ks == 4 ? launch_wreg_k<EPI, 4, 3>(h, a) : launch_wreg_k<EPI, 6, 3>(h, a));
    return ks == 3 ? launch_wreg_k<EPI, 3, 2>(h, a) : (ks == 4 ? launch_wreg_k<EPI, 4, 2>(h, a) : launch_wreg_k<EPI, 6, 2>(h, a));
}

static GemmArgs linear_args(const int8_t *x, const int8_t *w, const int32_t *bias, int M, int N, int K) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = x; a.B = w; a.M = M; a.N = N; a.K = K;
    a.lda = K; a.ldb = K; a.ldc = N;
    a.inner = 1; a.bias = bias;
    return a;
}

extern "C" {

int ivit_linear_i8(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias, int32_t *acc,
                   int M, int N, int K) {
    CHECK_H(h);
    REQUIRE(h, x && w && acc && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (K % 16) == 0, "K must be a multiple of 16");
    REQUIRE_A16(h, x, "x");                 // acc: 32-bit scalar stores (gemm_nt_kernel, EPI_RAW32)
    REQUIRE_DISJOINT(h, x, (size_t)M * K, "x", acc, (size_t)M * N * 4, "acc", OVL_IN);
    GemmArgs a = linear_args(x, w, bias, M, N, K);
    a.out = acc;
    return launch_gemm<false, EPI_RAW32>(h, a, 1);
}

int ivit_linear_i8_requant(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                           const ivit_dyadic *dy_ch, int bits, void *out, int M, int N, int K) {
    CHECK_H(h);
    REQUIRE(h, x && w && out && dy_ch && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (K % 16) == 0, "K must be a multiple of 16");
    REQUIRE(h, bits == 8 || bits == 16, "bits must be 8 or 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out, "out");
    REQUIRE_DISJOINT(h, x, (size_t)M * K, "x", out, (size_t)M * N * (bits / 8), "out", OVL_IN);
    GemmArgs a = linear_args(x, w, bias, M, N, K);
    a.out = out; a.dy_ch = dy_ch;
    if (const int nct = wreg_nct(a)) return bits == 8 ? launch_wreg<EPI_RQ8_CH>(h, a, nct) : launch_wreg<EPI_RQ16_CH>(h, a, nct);
    if (use_gemm2(a)) return bits == 8 ? launch_gemm2<EPI_RQ8_CH>(h, a) : launch_gemm2<EPI_RQ16_CH>(h, a);
    return bits == 8 ? launch_gemm<false, EPI_RQ8_CH>(h, a, 1) : launch_gemm<false, EPI_RQ16_CH>(h, a, 1);
}

// QuantLinear -> QuantAct(8) whose consumer is the 16-bit stream: clamp to 8 bits, store int16 (the widening pass ivit_widen_i8_i16 folded
// into the GEMM's stores): the Swin runner's PatchMerging reduction
int ivit_linear_i8_requant8_store16(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias, const ivit_dyadic *dy_ch,
                                    int16_t *out, int M, int N, int K) {
    CHECK_H(h);
    REQUIRE(h, x && w && out && dy_ch && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (K % 16) == 0, "K must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out, "out16");
    REQUIRE_DISJOINT(h, x, (size_t)M * K, "x", out, (size_t)M * N * 2, "out16", OVL_IN);
    GemmArgs a = linear_args(x, w, bias, M, N, K);
    a.out = out; a.dy_ch = dy_ch;
    if (wreg_nct(a) || !use_gemm2(a)) {
        snprintf(h->err, sizeof(h->err), "%s: built for gemm_glds_kernel's shapes (use ivit_linear_i8_requant + ivit_widen_i8_i16)", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    return launch_gemm2<EPI_RQ8W16_CH>(h, a);
}

int ivit_linear_i8_requant_residual(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                                    const ivit_dyadic *dy_ch, ivit_dyadic dy_main, ivit_dyadic dy_res,
                                    const int16_t *residual, int16_t *out, int M, int N, int K) {
    CHECK_H(h);
    REQUIRE(h, x && w && out && dy_ch && residual && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (K % 16) == 0, "K must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, residual, "residual");
    REQUIRE_A16(h, out, "out");
    REQUIRE_DISJOINT(h, x, (size_t)M * K, "x", out, (size_t)M * N * 2, "out", OVL_IN);
    // residual == out is the in-place form x = x + f(x).  In gemm_nt_kernel and gemm_glds_kernel a lane loads the eight identity values
    // of (grow, gcol) under the same grow < M, gcol < N test as its store of those eight elements, load first; gemm_wreg_kernel's lane
    // loads the identity of its own row and channels ahead of the MFMAs and stores the same elements behind them, and a lane past M
    // loads row M - 1 but stores nothing (every store is under `live`).  No lane loads an element that another lane stores.
    REQUIRE_DISJOINT_OR_SAME(h, residual, (size_t)M * N * 2, "residual", out, (size_t)M * N * 2, "out", OVL_IN);
    GemmArgs a = linear_args(x, w, bias, M, N, K);
    a.out = out; a.dy_ch = dy_ch; a.dy_main = dy_main; a.dy_res = dy_res; a.residual = residual;
    if (const int nct = wreg_nct(a)) return launch_wreg<EPI_RQ16_CH_RES>(h, a, nct);
    if (use_gemm2(a)) return launch_gemm2<EPI_RQ16_CH_RES>(h, a);
    return launch_gemm<false, EPI_RQ16_CH_RES>(h, a, 1);
}

int ivit_linear_i8_qkv(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                       const ivit_dyadic *dy_ch, int8_t *q, int8_t *k, int8_t *vt, int B, int T, int H,
                       int dh, int ldv) {
    CHECK_H(h);
    REQUIRE(h, x && w && dy_ch && q && k && vt && B > 0 && T > 0 && H > 0 && dh > 0, "bad arguments");
    REQUIRE(h, (dh % 16) == 0, "head dim must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_A16(h, vt, "vt");
    REQUIRE(h, ldv == 0 || ldv >= T, "ldv < T (0 = v row-major [B*H, T, dh])");
    const int D = H * dh;
    if (int st = qkv_disjoint(h, __func__, x, (size_t)B * T * D, "x", q, k, vt, B, T, H, dh, ldv)) return st;
    GemmArgs a = linear_args(x, w, bias, B * T, 3 * D, D);
    a.dy_ch = dy_ch; a.q = q; a.k = k; a.vt = vt;
    a.T = T; a.H = H; a.dh = dh; a.ldv = ldv; a.D = D;
    if (use_gemm2(a) && (dh % 16) == 0)
        return launch_gemm2<EPI_QKV>(h, a);
    return launch_gemm<false, EPI_QKV>(h, a, 1);
}

int ivit_bmm_nt_i8(ivit_handle h, const int8_t *A, const int8_t *B, int32_t *C, int nb, int M, int N, int K,
                   int lda, int ldb, int ldc, int64_t strideA, int64_t strideB, int64_t strideC) {
    CHECK_H(h);
    REQUIRE(h, A && B && C && nb > 0 && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (lda % 16) == 0 && (ldb % 16) == 0 && (strideA % 16) == 0 && (strideB % 16) == 0,
            "lda/ldb/strides must be multiples of 16");
    REQUIRE_A16(h, A, "A");                 // C: 32-bit scalar stores (gemm_nt_kernel, EPI_RAW32)
    REQUIRE_A16(h, B, "B");
    if (int st = bmm_disjoint(h, __func__, A, 1, B, C, nb, M, N, K, lda, ldb, ldc, strideA, strideB, strideC)) return st;
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.strideA = strideA; a.strideB = strideB; a.inner = 1; a.sC_outer = strideC; a.out = C;
    return launch_gemm<false, EPI_RAW32>(h, a, nb);
}

int ivit_bmm_nt_u16i8(ivit_handle h, const uint16_t *A, const int8_t *B, int32_t *C, int nb, int M, int N,
                      int K, int lda, int ldb, int ldc, int64_t strideA, int64_t strideB, int64_t strideC) {
    CHECK_H(h);
    REQUIRE(h, A && B && C && nb > 0 && M > 0 && N > 0 && K > 0, "bad arguments");
    REQUIRE(h, (lda % 8) == 0 && (ldb % 16) == 0 && (strideA % 8) == 0 && (strideB % 16) == 0,
            "lda must be a multiple of 8, ldb of 16");
    REQUIRE_A16(h, A, "A");
    REQUIRE_A16(h, B, "B");
    if (int st = bmm_disjoint(h, __func__, A, 2, B, C, nb, M, N, K, lda, ldb, ldc, strideA, strideB, strideC)) return st;
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.strideA = strideA; a.strideB = strideB; a.inner = 1; a.sC_outer = strideC; a.out = C;
    return launch_gemm<true, EPI_RAW32>(h, a, nb);
}

int ivit_attn_qk_requant(ivit_handle h, const int8_t *q, const int8_t *k, ivit_dyadic dy, int8_t *scores8,
                         int BH, int T, int dh, int lds) {
    CHECK_H(h);
    REQUIRE(h, q && k && scores8 && BH > 0 && T > 0 && dh > 0, "bad arguments");
    REQUIRE(h, (dh % 16) == 0 && lds >= T, "dh %16, lds >= T");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_A16(h, scores8, "scores8");
    REQUIRE_DISJOINT(h, q, (size_t)BH * T * dh, "q", scores8, span_bytes((long long)BH * T, lds, T, 1), "scores8", OVL_IN);
    REQUIRE_DISJOINT(h, k, (size_t)BH * T * dh, "k", scores8, span_bytes((long long)BH * T, lds, T, 1), "scores8", OVL_IN);
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = q; a.B = k; a.M = T; a.N = T; a.K = dh; a.lda = dh; a.ldb = dh; a.ldc = lds;
    a.strideA = (long long)T * dh; a.strideB = (long long)T * dh;
    a.inner = 1; a.sC_outer = (long long)T * lds; a.out = scores8; a.dy_main = dy;
    return launch_gemm<false, EPI_RQ8_S>(h, a, BH);
}

int ivit_attn_pv_requant(ivit_handle h, const uint16_t *p, const int8_t *vt, ivit_dyadic dy, int8_t *ctx8,
                         int B, int H, int T, int dh, int ldp, int ldv) {
    CHECK_H(h);
    REQUIRE(h, p && vt && ctx8 && B > 0 && H > 0 && T > 0 && dh > 0, "bad arguments");
    REQUIRE(h, (ldp % 8) == 0 && (ldv % 16) == 0 && ldp >= T && ldv >= T, "ldp %8, ldv %16, >= T");
    REQUIRE_A16(h, p, "p");
    REQUIRE_A16(h, vt, "vt");
    REQUIRE_A16(h, ctx8, "ctx8");
    REQUIRE_DISJOINT(h, p, span_bytes((long long)B * H * T, ldp, T, 2), "p", ctx8, (size_t)B * T * H * dh, "ctx8", OVL_IN);
    REQUIRE_DISJOINT(h, vt, span_bytes((long long)B * H * dh, ldv, T, 1), "vt", ctx8, (size_t)B * T * H * dh, "ctx8", OVL_IN);
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = p; a.B = vt; a.M = T; a.N = dh; a.K = T; a.lda = ldp; a.ldb = ldv; a.ldc = H * dh;
    a.strideA = (long long)T * ldp; a.strideB = (long long)dh * ldv;
    a.inner = H; a.sC_outer = (long long)T * H * dh; a.sC_inner = dh; a.out = ctx8; a.dy_main = dy;
    return launch_gemm<true, EPI_RQ8_S>(h, a, B * H);
}

}  // extern "C"



// ---------------------------------------------------------------- constants: upload / RCCL broadcast
extern "C" {

int ivit_constants_upload(ivit_handle h, const void *host_blob, size_t bytes, void *device_blob) {
    CHECK_H(h);
    REQUIRE(h, host_blob && device_blob && bytes > 0, "bad arguments");
    hipError_t e = hipMemcpyAsync(device_blob, host_blob, bytes, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "ivit_constants_upload: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    return IVIT_OK;
}

// ncclBroadcast(sendbuff, recvbuff, count, datatype, root, comm, stream) resolved from librccl.so at first use, so that
// libivit_hip.so itself carries no link-time dependency on RCCL (single-GPU users never load it)
int ivit_constants_broadcast(ivit_handle h, void *device_blob, size_t bytes, int root, void *rccl_comm) {
    CHECK_H(h);
    REQUIRE(h, device_blob && rccl_comm && bytes > 0 && root >= 0, "bad arguments");
    typedef int (*bcast_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
    static bcast_fn fn = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        void *lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (lib) fn = (bcast_fn)dlsym(lib, "ncclBroadcast");
    });
    if (!fn) { snprintf(h->err, sizeof(h->err), "ivit_constants_broadcast: librccl.so / ncclBroadcast not found"); return IVIT_ERR_UNSUPPORTED; }
    const int rc = fn(device_blob, device_blob, bytes, /* ncclUint8 */ 1, root, rccl_comm, h->stream);   // in place: one ring over xGMI
    if (rc != 0) { snprintf(h->err, sizeof(h->err), "ivit_constants_broadcast: ncclBroadcast returned %d", rc); return IVIT_ERR_HIP; }
    return IVIT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- linear plans (frozen QuantLinear)
// One wavefront per output channel: c[n] = m*2^-e, zmax[n] = 128 * sum_k |W[n,k]| + |bias[n]| >= |acc + bias|.
// bad bit 0: |zmax * c| >= 2^31 (the magic-number rounding of the pipelined epilogue could wrap);
// bad bit 1: zmax * |m| >= 2^53 (z*m inexact in fp64: the single-FMA form is not the reference's two roundings).
__global__ __launch_bounds__(256) void linear_plan_kernel(const int8_t *__restrict__ w, const int32_t *__restrict__ bias,
                                                          const ivit_dyadic *__restrict__ dy, int N, int K,
                                                          double *__restrict__ cq, int *__restrict__ bad) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int8_t *wp = w + (long long)n * K;
    int l1 = 0;
    for (int k = lane; k < K; k += 64) l1 += abs((int)wp[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l1 += __shfl_xor(l1, o);
    if (lane == 0) {
        const double c = dy[n].m * dy[n].r;
        cq[n] = c;
        const double zmax = 128.0 * (double)l1 + fabs((double)(bias ? bias[n] : 0));
        int b = 0;
        if (!rq_magic_safe(c, zmax)) b |= 1;
        if (!(fabs(dy[n].m) * zmax < 9007199254740992.0)) b |= 4;      // bound fails: linear_plan_fma_kernel decides
        if (b) atomicOr(bad, b);
    }
}

// Channels whose |z * m| may exceed 2^53 (the cheap bound above failed, flag 4): is the one-FMA requant
//   f1(z) = lo32(fma(double(z), c, 1.5 * 2^52)) = RNE(z * c)            (one rounding)
// still the reference's  f2(z) = RNE(fl64(z * m) * 2^-e)                (two roundings, quant_utils.py:229-231)  on [-zmax, zmax]?
// Both are non-decreasing step functions of the integer z; they agree on the clamped 16-bit range (and so on the 8-bit one)
// iff every step of f1 into a value k in (-32768, 32768] is a step of f2 at the same z.  One block per channel, 65536 steps
// over 256 threads; steps whose |z * m| < 2^53 are exact in both and skipped.  A failing channel sets flag 2.
__global__ __launch_bounds__(256) void linear_plan_fma_kernel(const int8_t *__restrict__ w, const int32_t *__restrict__ bias,
                                                              const ivit_dyadic *__restrict__ dy, int N, int K, int *__restrict__ bad) {
    __shared__ int s_l1, s_fail;
    const int n = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_l1 = 0; s_fail = 0; }
    __syncthreads();
    int l1 = 0;
    for (int k = tid; k < K; k += 256) l1 += abs((int)w[(long long)n * K + k]);
    atomicAdd(&s_l1, l1);
    __syncthreads();
    const double m = dy[n].m, r = dy[n].r, c = m * r;
    const double zmax = 128.0 * (double)s_l1 + fabs((double)(bias ? bias[n] : 0));
    if (fabs(m) * zmax < 9007199254740992.0) return;               // exact products: nothing to prove
    if (!(c > 0.0) || !rq_magic_safe(1.0, zmax)) { if (tid == 0) atomicOr(bad, 2); return; }      // (|z| itself must fit the bound)
    auto f1 = [&](double z) { return __double2loint(__builtin_fma(z, c, RQ_MAGIC)); };
    auto f2 = [&](double z) { return (int)__builtin_rint((z * m) * r); };
    bool fail = false;
    for (int i = 0; i < 256 && !fail; ++i) {
        const int k = -32767 + tid + 256 * i;                        // step INTO k
        double z0 = __builtin_ceil(((double)k - 0.5) / c);
        for (int it = 0; it < 4 && z0 - 1.0 >= -zmax && f1(z0 - 1.0) >= k; ++it) z0 -= 1.0;
        for (int it = 0; it < 4 && z0 <= zmax && f1(z0) < k; ++it) z0 += 1.0;
        if (fabs(z0) * fabs(m) < 9.0e15) continue;                   // |z * m| < 2^53 around this step
        if (z0 <= zmax && z0 >= -zmax && (f1(z0) < k || f2(z0) < k)) fail = true;
        if (z0 - 1.0 <= zmax && z0 - 1.0 >= -zmax && (f1(z0 - 1.0) >= k || f2(z0 - 1.0) >= k)) fail = true;
    }
    if (fail) atomicOr(&s_fail, 1);
    __syncthreads();
    if (tid == 0 && s_fail) atomicOr(bad, 2);
}

struct ivit_linear_plan_s {
    const int8_t *w;
    const int32_t *bias;        // caller's pointer (may be null)
    const int32_t *bias_eff;    // never null: zeros inside `dev` when the layer has no bias
    const ivit_dyadic *dy;
    int N, K;
    char *dev;                  // one allocation: cq[N] doubles | zero bias (optional) | flag word | 1 KB store scratch
    double *cq;
    void *dummy;
    int pipelined_ok, single_fma_ok;
    v4i *wf;                    // ivit_linear_plan_prepare_ws: the weights in gemm_ws_qkv_kernel's fragment order (own allocation), or null
    int device;                 // where `dev` lives: destroy / debug reads run there whatever the caller's current device is
};

extern "C" {

int ivit_linear_plan_create(ivit_handle h, const int8_t *w, const int32_t *bias, const ivit_dyadic *dy_ch, int N, int K,
                            ivit_linear_plan *out) {
    CHECK_H(h);
    REQUIRE(h, w && dy_ch && out && N > 0 && K > 0, "bad arguments");
    const size_t cq_bytes = ((size_t)N * 8 + 255) & ~(size_t)255, b_bytes = ((size_t)N * 4 + 255) & ~(size_t)255;
    char *dev = nullptr;
    hipError_t e = hipMalloc((void **)&dev, cq_bytes + b_bytes + 256 + 1024 + 8192);
    if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "ivit_linear_plan_create: hipMalloc: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    int *flag = (int *)(dev + cq_bytes + b_bytes);
    int host_bad = 3;
    bool ok = hipMemsetAsync(dev + cq_bytes, 0, b_bytes + 256 + 1024 + 8192, h->stream) == hipSuccess;
    if (ok) {
        linear_plan_kernel<<<(N + 3) / 4, 256, 0, h->stream>>>(w, bias, dy_ch, N, K, (double *)dev, flag);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(&host_bad, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;      // plan creation is a build-time call
    if (ok && (host_bad & 4) && !(host_bad & 1)) {                 // the cheap one-FMA bound failed somewhere: exact proof per channel
        linear_plan_fma_kernel<<<N, 256, 0, h->stream>>>(w, bias, dy_ch, N, K, flag);
        ok = hipGetLastError() == hipSuccess;
        ok = ok && hipMemcpyAsync(&host_bad, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
    } else if (host_bad & 4) {
        host_bad |= 2;
    }
    if (!ok) {
        snprintf(h->err, sizeof(h->err), "ivit_linear_plan_create: HIP error");
        (void)hipFree(dev);
        return IVIT_ERR_HIP;
    }
    ivit_linear_plan_s *p = new (std::nothrow) ivit_linear_plan_s();
    if (!p) { (void)hipFree(dev); return IVIT_ERR_HIP; }
    p->w = w; p->bias = bias; p->dy = dy_ch; p->N = N; p->K = K; p->dev = dev; p->cq = (double *)dev;
    p->bias_eff = bias ? bias : (const int32_t *)(dev + cq_bytes);
    p->dummy = dev + cq_bytes + b_bytes + 256;
    p->pipelined_ok = !(host_bad & 1);
    p->single_fma_ok = !(host_bad & 2);
    p->device = h->device;
    p->wf = nullptr;
    *out = p;
    return IVIT_OK;
}

int ivit_linear_plan_destroy(ivit_linear_plan p) {
    if (!p) return IVIT_ERR_INVALID;
    ivit_device_guard g;
    if (!g.enter(p->device)) return IVIT_ERR_HIP;
    (void)hipFree(p->dev);
    if (p->wf) (void)hipFree(p->wf);
    delete p;
    return IVIT_OK;
}

int ivit_linear_plan_query(ivit_linear_plan p, int *pipelined_ok, int *single_fma_ok) {
    if (!p) return IVIT_ERR_INVALID;
    if (pipelined_ok) *pipelined_ok = p->pipelined_ok;
    if (single_fma_ok) *single_fma_ok = p->single_fma_ok;
    return IVIT_OK;
}

}  // extern "C"

// persistent pipelined kernel: shapes it is built for (anything else runs on gemm_glds_kernel / gemm_nt_kernel).
// epi_bit: the epilogue asking — 1 requant (8/16-bit), 2 qkv scatter, 4 requant + residual
static inline bool use_gemm3(const ivit_linear_plan_s *pl, const GemmArgs &a, int epi_bit) {
    // the residual flavour on a narrow output (N = 384: three channel tiles per 256-token panel, 77 % balance, and its
    // 32 resident residual registers) measured no better in-model than the launch-per-tile kernel: N >= 512 only
    constexpr int res_min_n = 512;      // residual flavour on the persistent kernel from this output width on
    if (epi_bit == 4 && a.N < res_min_n) return false;
    return pl->pipelined_ok && (a.K % 64) == 0 && a.K >= 320 && (a.N % 16) == 0 && (a.ldc % 16) == 0 &&
           (a.lda % 16) == 0 && (a.ldb % 16) == 0 && a.M >= 128;
}

// ---- D = 384 / 192 qkv, plain 8-bit and proj + residual layers on the register-resident-weights kernel (ivit_gemm_ws.h), with or
// without norm1 in its prologue.  ldv = 0: v row-major; ldv >= T: v^T (the K = 192 geometry only)
static inline bool ws_plan_ok(const ivit_linear_plan_s *pl, long long M) { return pl->wf && ws_width(pl->K) && M < (1 << 26); }
static inline bool qkv_ws_ok(const ivit_linear_plan_s *pl, int B, int T, int H, int dh, int ldv = 0) {
    if (!(pl->wf && dh == 64 && ws_width(pl->K) && pl->N == 3 * H * dh && pl->N % 192 == 0 && (long long)B * H * T * 64 < (1ll << 31) &&
          (long long)B * T < (1ll << 26)))
        return false;
    return ldv == 0 || (pl->K == Ws192Geo::K && ldv >= T && ldv % 16 == 0 && (long long)B * H * 64 * ldv < (1ll << 31));
}
// one workgroup per CU of the handle's share, each with a contiguous range of 32-token tiles
template <class G, bool LN, int EPI, bool VT = false>
static int ws_launch(ivit_handle h, const ivit_linear_plan_s *pl, const WsArgs &a) {
    const int ntt = (a.M + 31) / 32;
    const unsigned grid = (unsigned)(ntt < persistent_cus(h) ? ntt : persistent_cus(h));
    return with_bool(pl->single_fma_ok, [&](auto FMA) {
        return launch_dyn<gemm_ws_qkv_kernel<G, FMA(), LN, EPI, VT>>(h, grid, WS_THREADS, G::SMEM, a);
    });
}
template <class G>
static int launch_qkv_ws_g(ivit_handle h, const ivit_linear_plan_s *pl, const int8_t *x8, const int16_t *x16, float ln_s,
                           const float *ln_bias_int, const float *ln_sc, const ivit_dyadic *ln_dy, int8_t *q, int8_t *k, int8_t *v,
                           int B, int T, int H, int ldv) {
    if (h->device != pl->device) { snprintf(h->err, sizeof(h->err), "qkv: plan and handle live on different devices"); return IVIT_ERR_INVALID; }
    if (ldv != 0 && !G::VT) { snprintf(h->err, sizeof(h->err), "qkv: no v^T store form at K = %d", G::K); return IVIT_ERR_UNSUPPORTED; }
    WsArgs a;
    a.x = x8; a.wf = pl->wf; a.bias = pl->bias_eff; a.cq = pl->cq; a.q = q; a.k = k; a.v = v;
    a.M = B * T; a.N = pl->N; a.T = T; a.H = H; a.dummy = pl->dummy;
    a.x16 = x16; a.ln_s = ln_s; a.ln_bias_int = ln_bias_int; a.ln_sc = ln_sc; a.ln_dy = ln_dy;
    a.residual = nullptr; a.out16 = nullptr; a.cm = a.cr = 0.0; a.ln_out8 = nullptr; a.ldv = ldv;
    if (H == 0) { a.T = 1; a.H = 1; }      // plain 8-bit output [M][N] (q = out8; T = 1)
    const int st = with_bool(x16 != nullptr, [&](auto LN) {
        if (H == 0) return ws_launch<G, LN(), WS_EPI_RQ8>(h, pl, a);
        if constexpr (G::VT) {
            if (ldv != 0) return ws_launch<G, LN(), WS_EPI_QKV8, true>(h, pl, a);
        }
        return ws_launch<G, LN(), WS_EPI_QKV8>(h, pl, a);
    });
    if (st) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}
static int launch_qkv_ws(ivit_handle h, const ivit_linear_plan_s *pl, const int8_t *x8, const int16_t *x16, float ln_s,
                         const float *ln_bias_int, const float *ln_sc, const ivit_dyadic *ln_dy, int8_t *q, int8_t *k, int8_t *v,
                         int B, int T, int H, int ldv = 0) {
    return pl->K == Ws192Geo::K ? launch_qkv_ws_g<Ws192Geo>(h, pl, x8, x16, ln_s, ln_bias_int, ln_sc, ln_dy, q, k, v, B, T, H, ldv)
                                : launch_qkv_ws_g<Ws384Geo>(h, pl, x8, x16, ln_s, ln_bias_int, ln_sc, ln_dy, q, k, v, B, T, H, ldv);
}

template <class G>
static int launch_res_ws_g(ivit_handle h, const ivit_linear_plan_s *pl, const int8_t *x8, ivit_dyadic dy_main, ivit_dyadic dy_res, const int16_t *residual,
                           int16_t *out, int M, float ln_s, const float *ln_bias_int, const float *ln_sc, const ivit_dyadic *ln_dy,
                           int8_t *ln_out8) {
    constexpr bool TAIL = G::K == 384;      // norm2 in the launch's tail: built at 384 only
    if (h->device != pl->device) { snprintf(h->err, sizeof(h->err), "linear: plan and handle live on different devices"); return IVIT_ERR_INVALID; }
    if (ln_out8 && !TAIL) { snprintf(h->err, sizeof(h->err), "linear: no LayerNorm tail at K = %d", G::K); return IVIT_ERR_UNSUPPORTED; }
    WsArgs a;
    a.x = x8; a.wf = pl->wf; a.bias = pl->bias_eff; a.cq = pl->cq; a.q = a.k = a.v = nullptr;
    a.M = M; a.N = pl->N; a.T = 1; a.H = 1; a.dummy = pl->dummy;
    a.x16 = nullptr; a.ln_s = ln_s; a.ln_bias_int = ln_bias_int; a.ln_sc = ln_sc; a.ln_dy = ln_dy;
    a.residual = residual; a.out16 = out; a.cm = dy_main.m * dy_main.r; a.cr = dy_res.m * dy_res.r; a.ln_out8 = ln_out8; a.ldv = 0;
    int st = IVIT_OK;
    if (!ln_out8) st = ws_launch<G, false, WS_EPI_RES16>(h, pl, a);
    else if constexpr (TAIL) st = ws_launch<G, true, WS_EPI_RES16>(h, pl, a);
    if (st) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}
static int launch_res_ws(ivit_handle h, const ivit_linear_plan_s *pl, const int8_t *x8, ivit_dyadic dy_main, ivit_dyadic dy_res, const int16_t *residual,
                         int16_t *out, int M, float ln_s = 0.f, const float *ln_bias_int = nullptr, const float *ln_sc = nullptr,
                         const ivit_dyadic *ln_dy = nullptr, int8_t *ln_out8 = nullptr) {
    return pl->K == Ws192Geo::K ? launch_res_ws_g<Ws192Geo>(h, pl, x8, dy_main, dy_res, residual, out, M, ln_s, ln_bias_int, ln_sc, ln_dy, ln_out8)
                                : launch_res_ws_g<Ws384Geo>(h, pl, x8, dy_main, dy_res, residual, out, M, ln_s, ln_bias_int, ln_sc, ln_dy, ln_out8);
}

template <int EPI>
static int launch_gemm3(ivit_handle h, const ivit_linear_plan_s *pl, GemmArgs &a) {
    a.tiles_n = (a.N + 127) / 128;
    a.cq = pl->cq;
    a.bias = pl->bias_eff;
    a.dummy = pl->dummy;
    constexpr int wg_per_cu = 2;
    const bool fma = pl->single_fma_ok != 0;
    // gemm_as_kernel: K = n * 384; the qkv scatter additionally needs whole units inside one of q / k / v and whole
    // 32-channel groups inside one head.  Its operand offsets are 32-bit and its epilogue goes through buffer
    // resources (offsets < 2^31, out-of-range lanes parked at 0x80000000): larger tensors take the 64-bit kernels.
    const long long out_bytes = (EPI == EPI_QKV) ? std::max((long long)a.M * a.D, (long long)(a.M / (a.T > 0 ? a.T : 1) + 1) * a.D * a.ldv)
                                                 : (long long)a.M * a.ldc * ((EPI == EPI_RQ8_CH) ? 1 : 2);
    const bool astat = (a.K % (GA_BK * GA_NK)) == 0 && a.M >= 256 && (a.N % 32) == 0 &&
                       (long long)a.M * a.lda < (1LL << 32) && (long long)a.N * a.ldb < (1LL << 32) &&
                       out_bytes < (1LL << 31) &&
                       (EPI != EPI_QKV || ((a.D % 128) == 0 && (a.dh % 32) == 0));
    if (astat) {
        const long long nunits = (long long)((a.M + 255) / 256) * a.tiles_n;
        long long grid = h->num_cu;
        if (grid > nunits) grid = nunits;
        const dim3 g((unsigned)grid);
        with_bool(fma, [&](auto FMA) {
            if (a.K == GA_BK * GA_NK) gemm_as_kernel<EPI, false, FMA()><<<g, 512, 0, h->stream>>>(a);
            else gemm_as_kernel<EPI, true, FMA()><<<g, 512, 0, h->stream>>>(a);
        });
    } else {
        const long long nunits = (long long)((a.M + 127) / 128) * a.tiles_n;
        long long grid = (long long)h->num_cu * wg_per_cu;
        if (grid > nunits) grid = nunits;
        with_bool(fma, [&](auto FMA) { gemm_ps_kernel<EPI, FMA(), false><<<dim3((unsigned)grid), 256, 0, h->stream>>>(a); });
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" {

int ivit_linear_i8_requant_planned(ivit_handle h, ivit_linear_plan pl, const int8_t *x, int bits, void *out, int M) {
    CHECK_H(h);
    REQUIRE(h, pl && x && out && M > 0, "bad arguments");
    REQUIRE(h, bits == 8 || bits == 16, "bits must be 8 or 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out, "out");
    REQUIRE_DISJOINT(h, x, (size_t)M * pl->K, "x", out, (size_t)M * pl->N * (bits / 8), "out", OVL_IN);
    GemmArgs a = linear_args(x, pl->w, pl->bias, M, pl->N, pl->K);
    a.out = out; a.dy_ch = pl->dy;
    if (bits == 8 && ws_plan_ok(pl, M))      // prepared plan: tokens of a CU in LDS, weight slabs in registers
        return launch_qkv_ws(h, pl, x, nullptr, 0.f, nullptr, nullptr, nullptr, (int8_t *)out, nullptr, nullptr, M, 1, 0);
    if (use_gemm3(pl, a, 1)) return bits == 8 ? launch_gemm3<EPI_RQ8_CH>(h, pl, a) : launch_gemm3<EPI_RQ16_CH>(h, pl, a);
    return ivit_linear_i8_requant(h, x, pl->w, pl->bias, pl->dy, bits, out, M, pl->N, pl->K);
}

int ivit_layernorm_linear_i8_requant_planned(ivit_handle h, ivit_linear_plan pl, const int16_t *x16, float scale, const float *bias_int,
                                             const float *sc, const ivit_dyadic *ln_dy, int8_t *out8, int M) {
    CHECK_H(h);
    REQUIRE(h, pl && x16 && bias_int && sc && ln_dy && out8 && M > 0, "bad arguments");
    REQUIRE_A16(h, x16, "x16");
    REQUIRE_A16(h, out8, "out8");
    REQUIRE_DISJOINT(h, x16, (size_t)M * pl->K * 2, "x16", out8, (size_t)M * pl->N, "out8", OVL_IN);
    if (!ws_plan_ok(pl, M)) {
        snprintf(h->err, sizeof(h->err), "%s: needs ivit_linear_plan_prepare_ws on a K = 192 or 384 plan", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    return launch_qkv_ws(h, pl, nullptr, x16, scale, bias_int, sc, ln_dy, out8, nullptr, nullptr, M, 1, 0);
}

int ivit_linear_i8_requant_residual_planned(ivit_handle h, ivit_linear_plan pl, const int8_t *x, ivit_dyadic dy_main,
                                            ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int M) {
    CHECK_H(h);
    REQUIRE(h, pl && x && out && residual && M > 0, "bad arguments");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, residual, "residual");
    REQUIRE_A16(h, out, "out");
    REQUIRE_DISJOINT(h, x, (size_t)M * pl->K, "x", out, (size_t)M * pl->N * 2, "out", OVL_IN);
    // residual == out is refused on a plan, though the unplanned entry takes it: gemm_ps_kernel and gemm_as_kernel request a sub-tile's
    // identity pieces asynchronously, rounds ahead of its epilogue and at offsets clamped into the array for rows past M, and
    // gemm_ws_qkv_kernel's epilogue reads them per 32-token tile; that every such load is ordered before the store of its element by
    // the lane that owns it has not been shown for these three, and the launcher picks among them by shape
    REQUIRE_DISJOINT(h, residual, (size_t)M * pl->N * 2, "residual", out, (size_t)M * pl->N * 2, "out", OVL_IN);
    GemmArgs a = linear_args(x, pl->w, pl->bias, M, pl->N, pl->K);
    a.out = out; a.dy_ch = pl->dy; a.dy_main = dy_main; a.dy_res = dy_res; a.residual = residual;
    const bool res_fast = rq_fast2(dy_main, dy_res);
    if (res_fast && ws_plan_ok(pl, M)) return launch_res_ws(h, pl, x, dy_main, dy_res, residual, out, M);
    if (use_gemm3(pl, a, 4) && res_fast) return launch_gemm3<EPI_RQ16_CH_RES>(h, pl, a);
    return ivit_linear_i8_requant_residual(h, x, pl->w, pl->bias, pl->dy, dy_main, dy_res, residual, out, M, pl->N, pl->K);
}

int ivit_linear_i8_requant_residual_layernorm_planned(ivit_handle h, ivit_linear_plan pl, const int8_t *x, ivit_dyadic dy_main,
                                                      ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int M, float ln_scale,
                                                      const float *ln_bias_int, const float *ln_sc, const ivit_dyadic *ln_dy,
                                                      int8_t *ln_out8) {
    CHECK_H(h);
    REQUIRE(h, pl && x && out && residual && M > 0 && ln_bias_int && ln_sc && ln_dy && ln_out8, "bad arguments");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, residual, "residual");
    REQUIRE_A16(h, out, "out");
    REQUIRE_A16(h, ln_out8, "ln_out8");
    {   // residual == out included: the LayerNorm tail re-reads out through L1, where the identity loads may have left stale lines
        const size_t n16 = (size_t)M * pl->N * 2, n8 = (size_t)M * pl->N;
        REQUIRE_DISJOINT(h, x, (size_t)M * pl->K, "x", out, n16, "out", OVL_IN);
        REQUIRE_DISJOINT(h, x, (size_t)M * pl->K, "x", ln_out8, n8, "ln_out8", OVL_IN);
        REQUIRE_DISJOINT(h, residual, n16, "residual", out, n16, "out", OVL_IN);
        REQUIRE_DISJOINT(h, residual, n16, "residual", ln_out8, n8, "ln_out8", OVL_IN);
        REQUIRE_DISJOINT(h, out, n16, "out", ln_out8, n8, "ln_out8", OVL_OUT);
    }
    if (!(pl->wf && rq_fast2(dy_main, dy_res) && pl->K == Ws384Geo::K && pl->N == Ws384Geo::K && M < (1 << 26))) {
        snprintf(h->err, sizeof(h->err), "%s: needs ivit_linear_plan_prepare_ws on a 384 x 384 plan and residual multipliers in the fast range", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    return launch_res_ws(h, pl, x, dy_main, dy_res, residual, out, M, ln_scale, ln_bias_int, ln_sc, ln_dy, ln_out8);
}

int ivit_linear_i8_qkv_planned(ivit_handle h, ivit_linear_plan pl, const int8_t *x, int8_t *q, int8_t *k, int8_t *vt,
                               int B, int T, int H, int dh, int ldv) {
    CHECK_H(h);
    REQUIRE(h, pl && x && q && k && vt && B > 0 && T > 0 && H > 0 && dh > 0, "bad arguments");
    REQUIRE(h, (dh % 16) == 0, "head dim must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_A16(h, vt, "vt");
    REQUIRE(h, ldv == 0 || ldv >= T, "ldv < T (0 = v row-major [B*H, T, dh])");
    const int D = H * dh;
    REQUIRE(h, pl->N == 3 * D && pl->K == D, "plan shape is not [3*H*dh, H*dh]");
    if (int st = qkv_disjoint(h, __func__, x, (size_t)B * T * D, "x", q, k, vt, B, T, H, dh, ldv)) return st;
    GemmArgs a = linear_args(x, pl->w, pl->bias, B * T, 3 * D, D);
    a.dy_ch = pl->dy; a.q = q; a.k = k; a.vt = vt;
    a.T = T; a.H = H; a.dh = dh; a.ldv = ldv; a.D = D;
    if (qkv_ws_ok(pl, B, T, H, dh, ldv)) return launch_qkv_ws(h, pl, x, nullptr, 0.f, nullptr, nullptr, nullptr, q, k, vt, B, T, H, ldv);
    if (use_gemm3(pl, a, 2) && (long long)B * T < (1 << 23)) return launch_gemm3<EPI_QKV>(h, pl, a);
    return ivit_linear_i8_qkv(h, x, pl->w, pl->bias, pl->dy, q, k, vt, B, T, H, dh, ldv);
}

int ivit_linear_plan_prepare_ws(ivit_handle h, ivit_linear_plan pl) {
    CHECK_H(h);
    REQUIRE(h, pl, "null plan");
    REQUIRE(h, h->device == pl->device, "plan and handle live on different devices");
    if (pl->wf) return IVIT_OK;
    if (!ws_width(pl->K) || pl->N % 64 != 0 || pl->N > WS_MAXN || !pl->pipelined_ok) {
        snprintf(h->err, sizeof(h->err), "%s: built for K = 192 or 384, N a multiple of 64 up to %d, |(acc + bias) * c| < 2^31", __func__, WS_MAXN);
        return IVIT_ERR_UNSUPPORTED;
    }
    v4i *wf = nullptr;
    hipError_t e = hipMalloc((void **)&wf, (size_t)pl->N * pl->K);
    if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "%s: hipMalloc: %s", __func__, hipGetErrorString(e)); return IVIT_ERR_HIP; }
    ws_swizzle_kernel<<<64, 256, 0, h->stream>>>(pl->w, wf, pl->N, pl->K);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);       // plan preparation is a build-time call
    if (e != hipSuccess) { (void)hipFree(wf); snprintf(h->err, sizeof(h->err), "%s: %s", __func__, hipGetErrorString(e)); return IVIT_ERR_HIP; }
    pl->wf = wf;
    return IVIT_OK;
}

int ivit_layernorm_linear_i8_qkv_planned(ivit_handle h, ivit_linear_plan pl, const int16_t *x16, float scale, const float *bias_int,
                                         const float *sc, const ivit_dyadic *ln_dy, int8_t *q, int8_t *k, int8_t *v, int B, int T,
                                         int H, int dh) {
    return ivit_layernorm_linear_i8_qkv_ldv_planned(h, pl, x16, scale, bias_int, sc, ln_dy, q, k, v, B, T, H, dh, 0);     // v row-major
}

int ivit_layernorm_linear_i8_qkv_ldv_planned(ivit_handle h, ivit_linear_plan pl, const int16_t *x16, float scale, const float *bias_int,
                                             const float *sc, const ivit_dyadic *ln_dy, int8_t *q, int8_t *k, int8_t *vt, int B, int T,
                                             int H, int dh, int ldv) {
    CHECK_H(h);
    REQUIRE(h, pl && x16 && bias_int && sc && ln_dy && q && k && vt && B > 0 && T > 0 && H > 0 && dh > 0, "bad arguments");
    REQUIRE_A16(h, x16, "x16");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_A16(h, vt, "vt");
    REQUIRE(h, pl->N == 3 * H * dh && pl->K == H * dh, "plan shape is not [3*H*dh, H*dh]");
    REQUIRE(h, ldv == 0 || (ldv >= T && ldv % 16 == 0), "ldv: 0 (v row-major [B*H, T, dh]) or a multiple of 16 >= T (v^T)");
    if (int st = qkv_disjoint(h, __func__, x16, (size_t)B * T * H * dh * 2, "x16", q, k, vt, B, T, H, dh, ldv)) return st;
    if (!qkv_ws_ok(pl, B, T, H, dh, ldv)) {
        snprintf(h->err, sizeof(h->err), "%s: needs ivit_linear_plan_prepare_ws on a K = 192 or 384, dh = 64 plan, B*H*T*64 < 2^31, and K = 192 "
                                         "with B*H*64*ldv < 2^31 for v^T", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    return launch_qkv_ws(h, pl, nullptr, x16, scale, bias_int, sc, ln_dy, q, k, vt, B, T, H, ldv);
}

}  // extern "C"

// ---- fused Mlp (+ residual QuantAct) for D = 384, hidden = 1536 (ivit_mlp.h, ivit_mlp_rs.h), D = 256, hidden = 1024 and D = 192,
// hidden = 768 (ivit_mlp.h)
struct ivit_mlp_plan_s {
    ivit_linear_plan fc1, fc2;      // borrowed: must outlive this plan
    int width;                      // 384, 256 or 192
    v4i *w1f, *w2f;                 // fragment-ordered copies of the two weight matrices (one allocation)
    v4i *w1r, *w2r;                 // width 384: the same in the role-split kernel's order (ivit_mlp_rs.h), same allocation; else null
    int fma;                        // both layers: one fused rounding == the reference's two
    int kernel;                     // 0 = by shape, 1 = lock-step (mlp384_kernel / mlp256_kernel / mlp192_kernel), 2 = role-split (mlp384rs_kernel): ivit_mlp_plan_select
    int device;
};

extern "C" {

int ivit_mlp_plan_create(ivit_handle h, ivit_linear_plan fc1, ivit_linear_plan fc2, ivit_mlp_plan *out) {
    CHECK_H(h);
    REQUIRE(h, fc1 && fc2 && out, "null argument");
    const bool w384 = fc1->K == Mlp384Geo::C && fc1->N == Mlp384Geo::HD && fc2->K == Mlp384Geo::HD && fc2->N == Mlp384Geo::C;
    const bool w192 = fc1->K == Mlp192Geo::C && fc1->N == Mlp192Geo::HD && fc2->K == Mlp192Geo::HD && fc2->N == Mlp192Geo::C;
    const bool w256 = fc1->K == Mlp256Geo::C && fc1->N == Mlp256Geo::HD && fc2->K == Mlp256Geo::HD && fc2->N == Mlp256Geo::C;
    if (!w384 && !w256 && !w192) {
        snprintf(h->err, sizeof(h->err), "%s: built for 384 -> 1536 -> 384, 256 -> 1024 -> 256 and 192 -> 768 -> 192", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    if (!fc1->pipelined_ok || !fc2->pipelined_ok) {
        snprintf(h->err, sizeof(h->err), "%s: |(acc + bias) * c| < 2^31 not provable for these weights", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    // one fragment-ordered copy of each weight matrix for the lock-step kernel; width 384: two more for the role-split kernel
    const size_t wbytes = (size_t)fc1->K * fc1->N;
    char *dev = nullptr;
    if (hipMalloc((void **)&dev, (w384 ? 4 : 2) * wbytes) != hipSuccess) { snprintf(h->err, sizeof(h->err), "%s: hipMalloc failed", __func__); return IVIT_ERR_HIP; }
    if (w384) {
        mlp_swizzle_kernel<<<256, 256, 0, h->stream>>>(fc1->w, fc1->N, fc1->K, (v4i *)dev);
        mlp_swizzle_kernel<<<256, 256, 0, h->stream>>>(fc2->w, fc2->N, fc2->K, (v4i *)(dev + wbytes));
        rs_swizzle_w1_kernel<<<144, 256, 0, h->stream>>>(fc1->w, (v4i *)(dev + 2 * wbytes));
        rs_swizzle_w2_kernel<<<144, 256, 0, h->stream>>>(fc2->w, (v4i *)(dev + 3 * wbytes));
    } else if (w256) {
        mlp256_swizzle_kernel<<<256, 256, 0, h->stream>>>(fc1->w, fc1->N, fc1->K, (v4i *)dev);
        mlp256_swizzle_kernel<<<256, 256, 0, h->stream>>>(fc2->w, fc2->N, fc2->K, (v4i *)(dev + wbytes));
    } else {
        mlp192_swizzle_kernel<<<144, 256, 0, h->stream>>>(fc1->w, fc1->N, fc1->K, (v4i *)dev);
        mlp192_swizzle_kernel<<<144, 256, 0, h->stream>>>(fc2->w, fc2->N, fc2->K, (v4i *)(dev + wbytes));
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // plan creation is a build-time call
    ivit_mlp_plan_s *p = e == hipSuccess ? new (std::nothrow) ivit_mlp_plan_s() : nullptr;
    if (!p) {
        (void)hipFree(dev);
        snprintf(h->err, sizeof(h->err), "%s: %s", __func__, e == hipSuccess ? "out of memory" : hipGetErrorString(e));
        return IVIT_ERR_HIP;
    }
    p->fc1 = fc1; p->fc2 = fc2; p->width = fc1->K; p->w1f = (v4i *)dev; p->w2f = (v4i *)(dev + wbytes);
    p->w1r = w384 ? (v4i *)(dev + 2 * wbytes) : nullptr; p->w2r = w384 ? (v4i *)(dev + 3 * wbytes) : nullptr;
    p->fma = fc1->single_fma_ok && fc2->single_fma_ok;
    p->kernel = 0;
    p->device = h->device;
    *out = p;
    return IVIT_OK;
}

int ivit_mlp_plan_select(ivit_mlp_plan p, int kernel) {
    if (!p || kernel < 0 || kernel > 2) return IVIT_ERR_INVALID;
    if (p->width != Mlp384Geo::C && kernel == 2) return IVIT_ERR_UNSUPPORTED;      // widths 192 and 256 have the lock-step kernel only
    p->kernel = kernel;
    return IVIT_OK;
}

int ivit_mlp_plan_destroy(ivit_mlp_plan p) {
    if (!p) return IVIT_ERR_INVALID;
    ivit_device_guard g;
    if (!g.enter(p->device)) return IVIT_ERR_HIP;
    (void)hipFree(p->w1f);
    delete p;
    return IVIT_OK;
}

// width 384: does ivit_mlp_fused_planned run (plan, M tokens) on the role-split kernel?  Two kernels, the same integers.  The
// role-split one (producer waves on fc1 of unit u + 1 beside consumer waves on ShiftGELU / fc2 / epilogue of unit u) needs a second
// unit per workgroup to overlap anything: with one unit per CU it only ties with the lock-step kernel (45.0 vs 44.6 us at
// M = 20480), from two units on it wins (profiles/README.md, round 5)
static bool mlp_role_split(const ivit_ctx *h, ivit_mlp_plan p, long long M) {
    if (p->width != Mlp384Geo::C) return false;
    const long long ntiles = (M + 15) / 16, nunits = (ntiles + MLP_TT - 2) / (MLP_TT - 1);
    return p->kernel == 2 || (p->kernel == 0 && nunits > (long long)persistent_cus(h));
}
// what ivit_layernorm_mlp_lockstep_planned takes: a width the LayerNorm-headed lock-step kernel is built at (not 256: the Swin runner
// keeps norm2 as its own launch by measurement) and residual multipliers in the fast range
static bool ln_mlp_lockstep_ok(ivit_mlp_plan p, ivit_dyadic dy_main, ivit_dyadic dy_res) {
    return p && (p->width == Mlp192Geo::C || p->width == Mlp384Geo::C) && rq_fast2(dy_main, dy_res);
}
// THE rule for "this block's norm2 + Mlp is ONE launch at M tokens on handle h", and through which entry: run_slice and
// ivit_vit_fused_ln_mlp_blocks ask here.  The role-split kernel's LayerNorm head where ivit_mlp_fused_planned would run on that kernel
// (width 384, two units per CU or more), else the lock-step kernel's (widths 192 and 384, every token count:
// profiles/README.md, "Norm2 inside the lock-step fused Mlp launch")
enum { LN_MLP_TWO_LAUNCHES = 0, LN_MLP_ROLE_SPLIT = 1, LN_MLP_LOCKSTEP = 2 };
static int ln_mlp_plan_fuses(const ivit_ctx *h, ivit_mlp_plan p, ivit_dyadic dy_main, ivit_dyadic dy_res, long long M) {
    if (!p || !rq_fast2(dy_main, dy_res)) return LN_MLP_TWO_LAUNCHES;
    if (mlp_role_split(h, p, M)) return LN_MLP_ROLE_SPLIT;
    return ln_mlp_lockstep_ok(p, dy_main, dy_res) ? LN_MLP_LOCKSTEP : LN_MLP_TWO_LAUNCHES;
}

// ln_lockstep: norm2 in the lock-step kernel's activation tiles (ivit_layernorm_mlp_lockstep_planned: x is null, `residual` the
// LayerNorm's input too); the lock-step kernel whatever the plan is pinned to, same grids, same unit schedules
static int mlp_fused_launch(ivit_handle h, ivit_mlp_plan p, const int8_t *x, const int8_t *gelu_table, ivit_dyadic dy_main,
                            ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int64_t M, float ln_s, const float *ln_bias_int,
                            const float *ln_sc, const ivit_dyadic *ln_dy, bool ln_lockstep = false) {
    MlpArgs a;
    a.ln_s = ln_s; a.ln_bias_int = ln_bias_int; a.ln_sc = ln_sc; a.ln_dy = ln_dy;
    a.x = x; a.w1f = p->w1f; a.w2f = p->w2f; a.b1 = p->fc1->bias_eff; a.b2 = p->fc2->bias_eff;
    a.cq1 = p->fc1->cq; a.cq2 = p->fc2->cq; a.tab = gelu_table; a.residual = residual; a.out = out;
    a.cm = dy_main.m * dy_main.r; a.cr = dy_res.m * dy_res.r; a.M = M;
    if (!rq_fast2(dy_main, dy_res)) {
        snprintf(h->err, sizeof(h->err), "%s: residual multipliers out of the fast range", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE(h, h->device == p->device, "plan and handle live on different devices");
    const long long ntiles = (M + 15) / 16;
    if (p->width != Mlp384Geo::C) {
        // widths 192 and 256: WG_PER_CU workgroups per CU of the handle's share; workgroup b walks the tile range [T b / G, T (b + 1) / G).
        // Lock-step only (ivit_layernorm_mlp_fused_planned refuses these widths before it comes here)
        const bool w256 = p->width == Mlp256Geo::C;
        const long long slots = (long long)(w256 ? Mlp256Geo::WG_PER_CU : Mlp192Geo::WG_PER_CU) * persistent_cus(h);
        const unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
        a.balanced = 1;
        const int st = with_bool(p->fma, [&](auto FMA) {
            if (ln_lockstep) return launch_dyn<mlp192ln_kernel<FMA()>>(h, grid, Mlp192Geo::THREADS, Mlp192Geo::SMEM_LN, a);
            return w256 ? launch_dyn<mlp256_kernel<FMA()>>(h, grid, Mlp256Geo::THREADS, Mlp256Geo::SMEM, a)
                        : launch_dyn<mlp192_kernel<FMA()>>(h, grid, Mlp192Geo::THREADS, Mlp192Geo::SMEM, a);
        });
        if (st) return st;
        LAUNCH_CHECK(h);
        return IVIT_OK;
    }
    // width 384: one workgroup per CU.  64-token units round-robin unless cutting contiguous tile ranges into units of <= 5 tiles
    // saves a whole round (a unit costs a pass over both weight matrices whatever its size)
    const long long nunits = (ntiles + MLP_TT - 2) / (MLP_TT - 1);
    const unsigned grid = (unsigned)(nunits < persistent_cus(h) ? nunits : persistent_cus(h));
    const long long rounds_fixed = (nunits + grid - 1) / grid, rounds_bal = (ntiles + (long long)MLP_TT * grid - 1) / ((long long)MLP_TT * grid);
    a.balanced = rounds_bal < rounds_fixed;
    // two kernels, the same integers (mlp_role_split)
    const bool role_split = !ln_lockstep && mlp_role_split(h, p, M);
    if (ln_dy && !role_split && !ln_lockstep) {
        snprintf(h->err, sizeof(h->err), "%s: the LayerNorm prologue exists in the role-split kernel only (two units per CU or more)", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    if (role_split) { a.w1f = p->w1r; a.w2f = p->w2r; }
    const int st = with_bool(p->fma, [&](auto FMA) {
        if (ln_lockstep) return launch_dyn<mlp384ln_kernel<FMA()>>(h, grid, MLP_THREADS, Mlp384Geo::SMEM_LN, a);
        if (!role_split) return launch_dyn<mlp384_kernel<FMA()>>(h, grid, MLP_THREADS, MLP_SMEM, a);
        return ln_dy ? launch_dyn<mlp384rs_kernel<FMA(), 1>>(h, grid, RS_THREADS, RS_SMEM, a)
                     : launch_dyn<mlp384rs_kernel<FMA()>>(h, grid, RS_THREADS, RS_SMEM, a);
    });
    if (st) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ivit_mlp_fused at C = 128, hidden = 512 (Swin-B stage 0): the lock-step body on the caller's own operands (mlp128_kernel; nothing is
// kept between calls but the per-device LDS attribute), two workgroups per CU of the handle's share
static int mlp128_launch(ivit_handle h, const int8_t *x, const int8_t *w1, const int32_t *b1, const ivit_dyadic *dy1, const int8_t *gelu_table,
                         const int8_t *w2, const int32_t *b2, const ivit_dyadic *dy2, ivit_dyadic dy_main, ivit_dyadic dy_res,
                         const int16_t *residual, int16_t *out, int64_t M) {
    MlpArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w1f = reinterpret_cast<const v4i *>(w1); a.w2f = reinterpret_cast<const v4i *>(w2); a.b1 = b1; a.b2 = b2;
    a.cq1 = reinterpret_cast<const double *>(dy1); a.cq2 = reinterpret_cast<const double *>(dy2);
    a.tab = gelu_table; a.residual = residual; a.out = out;
    a.cm = dy_main.m * dy_main.r; a.cr = dy_res.m * dy_res.r; a.M = M; a.balanced = 1;
    if (!rq_fast2(dy_main, dy_res)) {
        snprintf(h->err, sizeof(h->err), "ivit_mlp_fused: residual multipliers out of the fast range at C = 128");
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE(h, (((uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)dy1 | (uintptr_t)dy2 | (uintptr_t)b1 | (uintptr_t)b2) & 15) == 0,
            "C = 128: w1, w2, b1, b2, dy1, dy2 must be 16-byte aligned");
    REQUIRE_A16(h, x, "x");
    REQUIRE_ALIGNED(h, residual, "residual", 8);
    REQUIRE_ALIGNED(h, out, "out", 8);
    const long long ntiles = (M + 15) / 16, slots = (long long)Mlp128Geo::WG_PER_CU * persistent_cus(h);
    if (int st = launch_dyn<mlp128_kernel>(h, (unsigned)(ntiles < slots ? ntiles : slots), Mlp128Geo::THREADS, Mlp128Geo::SMEM, a)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_mlp_fused_planned(ivit_handle h, ivit_mlp_plan p, const int8_t *x, const int8_t *gelu_table, ivit_dyadic dy_main,
                           ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int64_t M) {
    CHECK_H(h);
    REQUIRE(h, p && x && gelu_table && residual && out && M > 0, "bad arguments");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, residual, "residual");
    REQUIRE_A16(h, out, "out");
    // residual == out is refused: the lock-step and role-split kernels fetch a unit's identity rows in fc2's epilogue with rows past
    // M - 1 of a 16-token tile clamped to row M - 1, which another tile's lanes store
    REQUIRE_DISJOINT(h, x, (size_t)M * p->width, "x", out, (size_t)M * p->width * 2, "out", OVL_IN);
    REQUIRE_DISJOINT(h, residual, (size_t)M * p->width * 2, "residual", out, (size_t)M * p->width * 2, "out", OVL_IN);
    return mlp_fused_launch(h, p, x, gelu_table, dy_main, dy_res, residual, out, M, 0.f, nullptr, nullptr, nullptr);
}

int ivit_layernorm_mlp_fused_planned(ivit_handle h, ivit_mlp_plan p, const int16_t *x16, float scale, const float *bias_int, const float *sc,
                                     const ivit_dyadic *ln_dy, int8_t *scratch8, const int8_t *gelu_table, ivit_dyadic dy_main,
                                     ivit_dyadic dy_res, int16_t *out, int64_t M) {
    CHECK_H(h);
    REQUIRE(h, p && x16 && bias_int && sc && ln_dy && scratch8 && gelu_table && out && M > 0, "bad arguments");
    REQUIRE_A16(h, x16, "x16");
    REQUIRE_A16(h, scratch8, "scratch8");
    REQUIRE_A16(h, out, "out");
    {   // x16 is fetched twice, for the LayerNorm and for the identity branch, by different lanes at different times: no in-place form
        const size_t n16 = (size_t)M * p->width * 2, n8 = (size_t)M * p->width;
        REQUIRE_DISJOINT(h, x16, n16, "x16", scratch8, n8, "scratch8", OVL_IN);
        REQUIRE_DISJOINT(h, x16, n16, "x16", out, n16, "out", OVL_IN);
        REQUIRE_DISJOINT(h, scratch8, n8, "scratch8", out, n16, "out", OVL_OUT);
    }
    if (p->width != MLP_C) {
        snprintf(h->err, sizeof(h->err), "%s: the LayerNorm prologue exists at width 384 only", __func__);      // not at 192, not at 256
        return IVIT_ERR_UNSUPPORTED;
    }
    return mlp_fused_launch(h, p, scratch8, gelu_table, dy_main, dy_res, x16, out, M, scale, bias_int, sc, ln_dy);
}

int ivit_layernorm_mlp_lockstep_planned(ivit_handle h, ivit_mlp_plan p, const int16_t *x16, float scale, const float *bias_int, const float *sc,
                                        const ivit_dyadic *ln_dy, const int8_t *gelu_table, ivit_dyadic dy_main, ivit_dyadic dy_res,
                                        int16_t *out, int64_t M) {
    CHECK_H(h);
    REQUIRE(h, p && x16 && bias_int && sc && ln_dy && gelu_table && out && M > 0, "bad arguments");
    REQUIRE_A16(h, x16, "x16");
    REQUIRE_A16(h, out, "out");
    // every row of x16 is read twice, by different lanes at different times (LayerNorm one unit ahead, the identity branch in fc2's
    // epilogue), and rows past M - 1 of a tile are row M - 1 again: in place is not a form this launch has
    REQUIRE(h, out + (size_t)M * p->width <= x16 || x16 + (size_t)M * p->width <= out, "out must not overlap x16 (LayerNorm input and identity branch)");
    if (!ln_mlp_lockstep_ok(p, dy_main, dy_res)) {
        snprintf(h->err, sizeof(h->err), "%s: built at widths 192 and 384, for residual multipliers in the fast range", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    return mlp_fused_launch(h, p, nullptr, gelu_table, dy_main, dy_res, x16, out, M, scale, bias_int, sc, ln_dy, true);
}

}  // extern "C"

template <int NB, bool FAST, int TT = 0, int LUT = 0, bool VROW = false, bool CLS = false>
static int launch_attn2(ivit_handle h, const AttnArgs &a, int BH) {
    const size_t lds = AttCfg<NB>::SMEM + (LUT == 2 ? (size_t)ATT_ROWLINE_BYTES
                                                   : (LUT == 1 ? (size_t)((a.t_count + 3) & ~3) * 4 + (size_t)a.nc * 512 + 256 : 0));
    // (since round 6 every launch of the row-table form is above 64 KB)
    REQUIRE_LAUNCH(h, BH, ATT_WAVES * 64, 1);
    if (int st = launch_dyn<attn_fused_kernel<NB, FAST, TT, LUT, VROW, CLS>>(h, BH, ATT_WAVES * 64, lds, a)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

template <int NB>
static int launch_attn(ivit_handle h, const AttnArgs &a, int BH) {
    const bool fast = attn_fast(a.dy_qk, a.dy_pv);
    const bool lut = a.aq && a.et && a.cls;
    if (a.rowtab)       // row-line tables (ivit_attention_fused_rowlut): the multipliers were checked by the caller
        return with_bool(a.ldv == 0, [&](auto VROW) {       // v row-major, or v^T
            if (NB == 4 && a.T == 197) return launch_attn2<NB, true, 197, 2, VROW()>(h, a, BH);
            if (NB == 10 && a.T == 577) return launch_attn2<NB, true, 577, 2, VROW()>(h, a, BH);
            return launch_attn2<NB, true, 0, 2, VROW()>(h, a, BH);
        });
    if (fast) {
        if (NB == 4 && a.T == 197) return lut ? launch_attn2<NB, true, 197, true>(h, a, BH) : launch_attn2<NB, true, 197>(h, a, BH);
        if (NB == 10 && a.T == 577) return lut ? launch_attn2<NB, true, 577, true>(h, a, BH) : launch_attn2<NB, true, 577>(h, a, BH);
    }
    if (fast && lut) return launch_attn2<NB, true, 0, true>(h, a, BH);
    return fast ? launch_attn2<NB, true>(h, a, BH) : launch_attn2<NB, false>(h, a, BH);
}

// the class-token form (a.nq != 0): the same Shiftmax forms, token count at run time (one query tile per workgroup: the
// folded tile tests of the fixed-T instantiations have nothing to pay for)
template <int NB>
static int launch_attn_cls(ivit_handle h, const AttnArgs &a, int BH) {
    const bool fast = attn_fast(a.dy_qk, a.dy_pv);
    const bool lut = a.aq && a.et && a.cls;
    if (a.rowtab) return with_bool(a.ldv == 0, [&](auto VROW) { return launch_attn2<NB, true, 0, 2, VROW(), true>(h, a, BH); });
    if (fast && lut) return launch_attn2<NB, true, 0, 1, false, true>(h, a, BH);
    return fast ? launch_attn2<NB, true, 0, 0, false, true>(h, a, BH) : launch_attn2<NB, false, 0, 0, false, true>(h, a, BH);
}

// cls_out: ctx8 is the compact [B, H*dh] buffer of the class-token rows (ivit_attention_fused*_cls); x16 / x_cls: their identity rows
static int attention_fused_impl(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt, ivit_dyadic dy_qk,
                                float s_softmax, ivit_dyadic dy_pv, int8_t *ctx8, int B, int H, int T, int dh, int ldv,
                                const uint16_t *aq, const float *et, const uint8_t *cls, int nc, int t_count, int dmin,
                                const float *rowtab = nullptr, bool cls_out = false, const int16_t *x16 = nullptr, int16_t *x_cls = nullptr) {
    CHECK_H(h);
    REQUIRE(h, q && k && vt && ctx8 && B > 0 && H > 0 && T > 0 && s_softmax > 0.f, "bad arguments");
    REQUIRE(h, (x16 == nullptr) == (x_cls == nullptr) && (cls_out || !x16), "x16 and x_cls go together (both null: no identity rows)");
    REQUIRE(h, !cls_out || (((uintptr_t)x16 | (uintptr_t)x_cls | (uintptr_t)ctx8) & 15) == 0, "ctx_cls, x16 and x_cls must be 16-byte aligned");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_A16(h, vt, "vt");
    REQUIRE_A16(h, ctx8, "ctx8");
    REQUIRE(h, ((ldv % 16) == 0 && ldv >= T) || (ldv == 0 && rowtab), "ldv must be a multiple of 16 and >= T (0 = v row-major: ivit_attention_fused_rowlut only)");
    if (dh > 0) {
        const char *oname = cls_out ? "ctx_cls" : "ctx8";
        const char *fn = rowtab ? (cls_out ? "ivit_attention_fused_rowlut_cls" : "ivit_attention_fused_rowlut")
                                : aq ? (cls_out ? "ivit_attention_fused_lut_cls" : "ivit_attention_fused_lut")
                                     : (cls_out ? "ivit_attention_fused_cls" : "ivit_attention_fused");
        const size_t nqk = (size_t)B * H * T * dh, nv = ldv == 0 ? nqk : span_bytes((long long)B * H * dh, ldv, T, 1);
        const size_t nctx = (size_t)B * (cls_out ? 1 : T) * H * dh, nx16 = (size_t)B * T * H * dh * 2, nxc = (size_t)B * H * dh * 2;
        const struct { const void *p; size_t n; const char *name; } in[4] = {{q, nqk, "q"}, {k, nqk, "k"}, {vt, nv, "vt"}, {x16, nx16, "x16"}};
        for (const auto &i : in)
            if (!ranges_disjoint(h, fn, i.p, i.n, i.name, ctx8, nctx, oname, OVL_IN) || !ranges_disjoint(h, fn, i.p, i.n, i.name, x_cls, nxc, "x_cls", OVL_IN))
                return IVIT_ERR_INVALID;
        if (!ranges_disjoint(h, fn, ctx8, nctx, oname, x_cls, nxc, "x_cls", OVL_OUT)) return IVIT_ERR_INVALID;
    }
    if (rowtab && !attn_fast(dy_qk, dy_pv)) {       // the row-table kernel is built with FAST = true only
        snprintf(h->err, sizeof(h->err), "ivit_attention_fused_rowlut%s: requant multipliers out of the fast range (use ivit_attention_fused_lut%s)",
                 cls_out ? "_cls" : "", cls_out ? "_cls" : "");
        return IVIT_ERR_UNSUPPORTED;
    }
    if (dh != 64 || T > 640) {
        snprintf(h->err, sizeof(h->err), "ivit_attention_fused: built for dh == 64, T <= 640");
        return IVIT_ERR_UNSUPPORTED;
    }
    if (aq) REQUIRE(h, et && cls && nc >= 1 && nc <= 64 && t_count >= 1 && t_count <= 16384 && dmin <= 0 && dmin >= -255,
                    "bad Shiftmax tables");
    if (aq) REQUIRE(h, (((uintptr_t)aq | (uintptr_t)et) & 15) == 0 && ((uintptr_t)cls & 3) == 0,
                    "Shiftmax tables: exp_aq and exp_t must be 16-byte aligned, exp_cls 4-byte aligned (copied in 16-byte pieces)");
    AttnArgs a;
    a.q = q; a.k = k; a.vt = vt; a.ctx = ctx8; a.T = T; a.H = H; a.ldv = ldv;
    a.s_softmax = s_softmax; a.dy_qk = dy_qk; a.dy_pv = dy_pv;
    a.aq = aq; a.et = et; a.cls = cls; a.nc = nc; a.t_count = t_count; a.dmin = dmin; a.rowtab = rowtab;
    a.nq = cls_out ? 1 : 0; a.ctx_rows = cls_out ? 1 : T; a.x16 = x16; a.x_cls = x_cls;
    if (cls_out) {
        if (T <= 64) return launch_attn_cls<1>(h, a, B * H);
        if (T <= 256) return launch_attn_cls<4>(h, a, B * H);
        return launch_attn_cls<10>(h, a, B * H);
    }
    if (T <= 64) return launch_attn<1>(h, a, B * H);
    if (T <= 256) return launch_attn<4>(h, a, B * H);
    return launch_attn<10>(h, a, B * H);
}

extern "C" int ivit_attention_fused(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                    ivit_dyadic dy_qk, float s_softmax, ivit_dyadic dy_pv, int8_t *ctx8, int B,
                                    int H, int T, int dh, int ldv) {
    return attention_fused_impl(h, q, k, vt, dy_qk, s_softmax, dy_pv, ctx8, B, H, T, dh, ldv, nullptr, nullptr, nullptr, 0, 0, 0);
}

extern "C" int ivit_attention_fused_lut(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                        ivit_dyadic dy_qk, float s_softmax, const uint16_t *exp_aq, const float *exp_t,
                                        const uint8_t *exp_cls, int nclass, int t_count, int dmin, ivit_dyadic dy_pv,
                                        int8_t *ctx8, int B, int H, int T, int dh, int ldv) {
    if (h && !(exp_aq && exp_t && exp_cls)) { snprintf(h->err, sizeof(h->err), "ivit_attention_fused_lut: null table"); return IVIT_ERR_INVALID; }
    return attention_fused_impl(h, q, k, vt, dy_qk, s_softmax, dy_pv, ctx8, B, H, T, dh, ldv, exp_aq, exp_t, exp_cls, nclass, t_count, dmin);
}

// rowtab[vmax + 128][dd] = exp_t[exp_aq[exp_cls[vmax]][v] + dd] for the score v = vmax + dmin + dd (dd = 0: every score at or
// below vmax + dmin, the floor constant of the table whatever the class); one thread per entry
__global__ __launch_bounds__(64) void shiftmax_rowtable_kernel(const uint16_t *__restrict__ aq, const float *__restrict__ et,
                                                               const uint8_t *__restrict__ cls, int dmin, float *__restrict__ rowtab) {
    const int q = blockIdx.x, dd = threadIdx.x, R = 1 - dmin;
    int vi = q + dmin + dd;
    float val = 0.f;
    if (dd < R && (vi >= 0 || dd == 0)) {
        vi = vi < 0 ? 0 : vi;
        val = et[(int)aq[(int)cls[q] * 256 + vi] + dd];
    }
    rowtab[q * 64 + dd] = val;
}

extern "C" int ivit_shiftmax_rowtable(ivit_handle h, const uint16_t *exp_aq, const float *exp_t, const uint8_t *exp_cls,
                                      int nclass, int t_count, int dmin, float *rowtab) {
    CHECK_H(h);
    REQUIRE(h, exp_aq && exp_t && exp_cls && rowtab && nclass >= 1 && nclass <= 64 && t_count >= 1 && t_count <= 16384 &&
                   dmin <= 0 && dmin >= -255, "bad Shiftmax tables");
    if (1 - dmin > 64) {
        snprintf(h->err, sizeof(h->err), "%s: a table line holds 64 entries, this scale needs %d (use ivit_attention_fused_lut)", __func__, 1 - dmin);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE(h, ((uintptr_t)rowtab & 15) == 0, "rowtab must be 16-byte aligned");
    shiftmax_rowtable_kernel<<<256, 64, 0, h->stream>>>(exp_aq, exp_t, exp_cls, dmin, rowtab);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// the row-table entries, whole T (cls_out false) and class-token form: a table line holds 64 entries and the kernel is built with
// FAST = true only
static int attention_rowlut(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt, ivit_dyadic dy_qk, float s_softmax,
                            const float *rowtab, int dmin, ivit_dyadic dy_pv, int8_t *ctx8, int B, int H, int T, int dh, int ldv,
                            bool cls_out, const int16_t *x16, int16_t *x_cls) {
    if (!h) return IVIT_ERR_INVALID;
    const char *entry = cls_out ? "ivit_attention_fused_rowlut_cls" : "ivit_attention_fused_rowlut";
    if (!(rowtab && ((uintptr_t)rowtab & 15) == 0 && dmin <= 0 && dmin >= -63)) {
        snprintf(h->err, sizeof(h->err), "%s: bad row table (16-byte aligned, 1 - dmin <= 64)", entry);
        return IVIT_ERR_INVALID;
    }
    if (!attn_fast(dy_qk, dy_pv)) {
        snprintf(h->err, sizeof(h->err), "%s: requant multipliers out of the fast range (use ivit_attention_fused_lut%s)", entry, cls_out ? "_cls" : "");
        return IVIT_ERR_UNSUPPORTED;
    }
    return attention_fused_impl(h, q, k, vt, dy_qk, s_softmax, dy_pv, ctx8, B, H, T, dh, ldv, nullptr, nullptr, nullptr, 0, 0, dmin, rowtab,
                                cls_out, x16, x_cls);
}

extern "C" int ivit_attention_fused_rowlut(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                           ivit_dyadic dy_qk, float s_softmax, const float *rowtab, int dmin, ivit_dyadic dy_pv,
                                           int8_t *ctx8, int B, int H, int T, int dh, int ldv) {
    return attention_rowlut(h, q, k, vt, dy_qk, s_softmax, rowtab, dmin, dy_pv, ctx8, B, H, T, dh, ldv, false, nullptr, nullptr);
}

// ---- the class-token forms: the context of token 0 of every image into ctx_cls [B, H*dh], its identity row of x16 into x_cls
extern "C" int ivit_attention_fused_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt, ivit_dyadic dy_qk,
                                        float s_softmax, ivit_dyadic dy_pv, int8_t *ctx_cls, const int16_t *x16, int16_t *x_cls,
                                        int B, int H, int T, int dh, int ldv) {
    return attention_fused_impl(h, q, k, vt, dy_qk, s_softmax, dy_pv, ctx_cls, B, H, T, dh, ldv, nullptr, nullptr, nullptr, 0, 0, 0,
                                nullptr, true, x16, x_cls);
}

extern "C" int ivit_attention_fused_lut_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt, ivit_dyadic dy_qk,
                                            float s_softmax, const uint16_t *exp_aq, const float *exp_t, const uint8_t *exp_cls,
                                            int nclass, int t_count, int dmin, ivit_dyadic dy_pv, int8_t *ctx_cls,
                                            const int16_t *x16, int16_t *x_cls, int B, int H, int T, int dh, int ldv) {
    if (h && !(exp_aq && exp_t && exp_cls)) { snprintf(h->err, sizeof(h->err), "%s: null table", __func__); return IVIT_ERR_INVALID; }
    return attention_fused_impl(h, q, k, vt, dy_qk, s_softmax, dy_pv, ctx_cls, B, H, T, dh, ldv, exp_aq, exp_t, exp_cls, nclass, t_count,
                                dmin, nullptr, true, x16, x_cls);
}

extern "C" int ivit_attention_fused_rowlut_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt, ivit_dyadic dy_qk,
                                               float s_softmax, const float *rowtab, int dmin, ivit_dyadic dy_pv, int8_t *ctx_cls,
                                               const int16_t *x16, int16_t *x_cls, int B, int H, int T, int dh, int ldv) {
    return attention_rowlut(h, q, k, vt, dy_qk, s_softmax, rowtab, dmin, dy_pv, ctx_cls, B, H, T, dh, ldv, true, x16, x_cls);
}

// out[r][:] = x[r * row_stride ...][:C]: `rows` rows of C 16-bit values, 16 bytes per thread (the stand-alone form of the identity-row
// copy that the class-token attention does on the side)
__global__ __launch_bounds__(256) void gather_rows16_kernel(const int16_t *__restrict__ x, long long row_stride, int C8, long long n,
                                                            int16_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long r = i / C8;
    const int c = (int)(i - r * C8);
    reinterpret_cast<v4i *>(out)[i] = *reinterpret_cast<const v4i *>(x + r * row_stride + c * 8);
}

extern "C" int ivit_gather_rows_i16(ivit_handle h, const int16_t *x, int64_t rows, int C, int64_t row_stride, int16_t *out) {
    CHECK_H(h);
    REQUIRE(h, x && out && rows > 0 && C > 0 && row_stride >= C, "bad arguments");
    REQUIRE(h, (C % 8) == 0 && (row_stride % 8) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0, "C and row_stride multiples of 8, x and out 16-byte aligned");
    const long long n = (long long)rows * (C / 8);
    REQUIRE(h, n < (1LL << 31) * 256, "too many rows");
    REQUIRE_DISJOINT(h, x, span_bytes(rows, row_stride, C, 2), "x", out, (size_t)rows * C * 2, "out", OVL_IN);
    REQUIRE_LAUNCH(h, (n + 255) / 256, 256, 256);
    gather_rows16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(x, row_stride, C / 8, n, out);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- requant
template <typename ZT>
static int requant_any(ivit_handle h, const char *fn, const ZT *z, const ivit_dyadic *dy, int nch, const int32_t *z_id,
                       const ivit_dyadic *dy_id, int bits, void *out, int64_t rows, int C) {
    const long long total = (long long)rows * C;
    {   // z == out is refused at every width: requant_kernel and requant_vec8_kernel declare z and out __restrict__
        const size_t nz = (size_t)total * sizeof(ZT), nout = (size_t)total * (bits / 8);
        if (!ranges_disjoint(h, fn, z, nz, "z", out, nout, "out", OVL_IN)) return IVIT_ERR_INVALID;
        if (!ranges_disjoint(h, fn, z_id, (size_t)total * 4, "z_id", out, nout, "out", OVL_IN)) return IVIT_ERR_INVALID;
    }
    // per-channel tables keep the element-per-lane form (coalesced constant loads), and so does an output that is not 16-byte aligned:
    // requant_vec8_kernel stores 8 (8-bit) or 16 (16-bit) bytes at once, requant_kernel one element.  Same integers
    if ((C % 8) == 0 && nch == 1 && ((uintptr_t)out & 15) == 0) {
        const int g8 = grid_for(h, total / 8, 256 * 2);
        if (bits == 8) requant_vec8_kernel<ZT, 8><<<g8, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total / 8, C / 8);
        else if (bits == 16) requant_vec8_kernel<ZT, 16><<<g8, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total / 8, C / 8);
        else requant_vec8_kernel<ZT, 32><<<g8, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total / 8, C / 8);
        LAUNCH_CHECK(h);
        return IVIT_OK;
    }
    const int g = grid_for(h, total, 256 * 4);
    if (bits == 8) requant_kernel<ZT, 8><<<g, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total, C);
    else if (bits == 16) requant_kernel<ZT, 16><<<g, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total, C);
    else requant_kernel<ZT, 32><<<g, 256, 0, h->stream>>>(z, dy, nch, z_id, dy_id, out, total, C);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" {

int ivit_requant_i32(ivit_handle h, const int32_t *z, const ivit_dyadic *dy, int nch, const int32_t *z_id,
                     const ivit_dyadic *dy_id, int bits, void *out, int64_t rows, int C) {
    CHECK_H(h);
    REQUIRE(h, z && dy && out && rows > 0 && C > 0, "bad arguments");
    REQUIRE(h, nch == 1 || nch == C, "nch must be 1 or C");
    REQUIRE(h, bits == 8 || bits == 16 || bits == 32, "bits must be 8, 16 or 32");
    REQUIRE(h, (z_id == nullptr) == (dy_id == nullptr), "z_id and dy_id go together");
    return requant_any<int32_t>(h, __func__, z, dy, nch, z_id, dy_id, bits, out, rows, C);
}

int ivit_requant_i16(ivit_handle h, const int16_t *z, const ivit_dyadic *dy, int nch, const int32_t *z_id,
                     const ivit_dyadic *dy_id, int bits, void *out, int64_t rows, int C) {
    CHECK_H(h);
    REQUIRE(h, z && dy && out && rows > 0 && C > 0, "bad arguments");
    REQUIRE(h, nch == 1 || nch == C, "nch must be 1 or C");
    REQUIRE(h, bits == 8 || bits == 16 || bits == 32, "bits must be 8, 16 or 32");
    REQUIRE(h, (z_id == nullptr) == (dy_id == nullptr), "z_id and dy_id go together");
    return requant_any<int16_t>(h, __func__, z, dy, nch, z_id, dy_id, bits, out, rows, C);
}

int ivit_requant_f32(ivit_handle h, const float *z, const ivit_dyadic *dy, int nch, const int32_t *z_id,
                     const ivit_dyadic *dy_id, int bits, void *out, int64_t rows, int C) {
    CHECK_H(h);
    REQUIRE(h, z && dy && out && rows > 0 && C > 0, "bad arguments");
    REQUIRE(h, nch == 1 || nch == C, "nch must be 1 or C");
    REQUIRE(h, bits == 8 || bits == 16 || bits == 32, "bits must be 8, 16 or 32");
    REQUIRE(h, (z_id == nullptr) == (dy_id == nullptr), "z_id and dy_id go together");
    return requant_any<float>(h, __func__, z, dy, nch, z_id, dy_id, bits, out, rows, C);
}

// ---------------------------------------------------------------- shift/norm kernels

int ivit_shiftmax(ivit_handle h, const int8_t *x, int64_t rows, int n, int ld_in, float scale, int out_bits,
                  uint16_t *out, int ld_out) {
    CHECK_H(h);
    REQUIRE(h, x && out && rows > 0 && n > 0 && ld_in >= n && ld_out >= n && scale > 0.f, "bad arguments");
    REQUIRE(h, out_bits == 8 || out_bits == 16, "out_bits must be 8 or 16");
    REQUIRE_DISJOINT(h, x, span_bytes(rows, ld_in, n, 1), "x", out, span_bytes(rows, ld_out, n, 2), "out", OVL_IN);
    const size_t lds = (size_t)4 * n * sizeof(float);
    REQUIRE(h, lds <= 160 * 1024, "row too long for LDS staging");
    REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4);
    if (int st = launch_dyn<shiftmax_kernel>(h, (unsigned)((rows + 3) / 4), 256, lds, x, rows, n, ld_in, scale, out_bits, out, ld_out)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// Host restatement of the product shiftgelu_kernel forms (same fp32 sequence, IEEE division; -ffp-contract=off holds for
// the host half too).  Q * sigmoid_int depends on (Q, row max) and the scale alone, so its extremes over the 32 896 pairs
// with Q <= row max are the extremes over every possible input.  Below a scale of about 1.2e-3 the reference's clamp of
// the exponential sum at 2^31 (quant_modules.py:437) lets sigmoid_int exceed 256 and the product leaves int16.
static float host_shift_exp(float x, float x0, float nx0, int n) {
    float t = x + floorf(x * 0.5f);
    t = t - floorf(x * 0.0625f);
    t = fmaxf(t, nx0);
    const float q = floorf(t / x0);
    const float r = t - x0 * q;
    float e = r * 0.5f - x0;
    e = floorf(ldexpf(e, n - (int)q));
    return fmaxf(e, 0.0f);
}

static void shiftgelu_product_range(float s, int *lo, int *hi) {
    static thread_local float cs = 0.f;      // the scale of a frozen layer repeats call after call
    static thread_local int clo = 0, chi = 0;
    if (s != cs) {
        const float x0 = floorf(-1.0f / (s * 1.702f)), nx0 = 23.0f * x0;
        float p[256];
        for (int q = -128; q < 128; ++q) p[q + 128] = ((float)q * s) / s;
        float mn = 0.f, mxv = 0.f;
        for (int qmax = -128; qmax < 128; ++qmax) {
            const float mx = p[qmax + 128];
            const float emax = host_shift_exp(-mx, x0, nx0, 23);
            for (int q = -128; q <= qmax; ++q) {
                const float e = host_shift_exp(p[q + 128] - mx, x0, nx0, 23);
                const float S = fminf(e + emax, 2147483648.0f);
                const float F = floorf((1.0f / S) * 2147483648.0f);
                const float sig = floorf((e * F) * 5.9604644775390625e-08f);
                const float prod = rintf(p[q + 128] * sig);
                mn = fminf(mn, prod);
                mxv = fmaxf(mxv, prod);
            }
        }
        clo = (int)fmaxf(mn, -2147483648.0f);
        chi = (int)fminf(mxv, 2147483520.0f);
        cs = s;
    }
    *lo = clo;
    *hi = chi;
}

int ivit_shiftgelu(ivit_handle h, const int8_t *x, int64_t rows, int C, float scale, int16_t *out16) {
    CHECK_H(h);
    REQUIRE(h, x && out16 && rows > 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE(h, (C % 16) == 0, "C must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out16, "out16");
    REQUIRE_DISJOINT(h, x, (size_t)rows * C, "x", out16, (size_t)rows * C * 2, "out16", OVL_IN);
    int lo, hi;
    shiftgelu_product_range(scale, &lo, &hi);
    if (lo < -32768 || hi > 32767) {
        snprintf(h->err, sizeof(h->err),
                 "ivit_shiftgelu: at scale %.9g Q*sigmoid_int spans [%d, %d] and does not fit the 16-bit output; use "
                 "ivit_shiftgelu_requant or the table form", (double)scale, lo, hi);
        return IVIT_ERR_UNSUPPORTED;
    }
    ivit_dyadic d = {0.0, 0.0};
    REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4);
    shiftgelu_kernel<false><<<(unsigned)((rows + 3) / 4), 256, 0, h->stream>>>(x, rows, C, scale, d, out16);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_shiftgelu_requant(ivit_handle h, const int8_t *x, int64_t rows, int C, float scale, ivit_dyadic dy,
                           int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && out8 && rows > 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE(h, (C % 16) == 0, "C must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out8, "out8");
    // x == out8 is refused like every other overlap: shiftgelu_kernel declares x and out __restrict__ and reads each chunk twice
    REQUIRE_DISJOINT(h, x, (size_t)rows * C, "x", out8, (size_t)rows * C, "out8", OVL_IN);
    REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4);
    shiftgelu_kernel<true><<<(unsigned)((rows + 3) / 4), 256, 0, h->stream>>>(x, rows, C, scale, dy, out8);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_shiftgelu_build_table(ivit_handle h, float scale, ivit_dyadic dy, int8_t *table) {
    CHECK_H(h);
    REQUIRE(h, table && scale > 0.f, "bad arguments");
    shiftgelu_table_kernel<<<256, 256, 0, h->stream>>>(scale, dy, table);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_shiftgelu_requant_lut(ivit_handle h, const int8_t *x, int64_t rows, int C, const int8_t *table,
                               int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && out8 && table && rows > 0 && C > 0, "bad arguments");
    REQUIRE(h, (C % 16) == 0, "C must be a multiple of 16");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out8, "out8");
    REQUIRE_DISJOINT(h, x, (size_t)rows * C, "x", out8, (size_t)rows * C, "out8", OVL_IN);
    // half a wavefront per row, row in registers: ITER = ceil(C / 512) chunks of 16 bytes per lane
    constexpr bool lut_old = false;
    const int iter = (C / 16 + 31) / 32;
    // The runtime takes a launch's global size (blocks x 256 threads) modulo 2^32 and runs the remainder WITHOUT an error (C = 16,
    // 134 221 828 rows: 513 of 16 777 729 blocks ran, the rows from 4104 on were never written): consecutive ranges of at most 2^25
    // rows go out as launches of their own, 2^22 (2^23) blocks each
    constexpr int64_t rows_per_launch = (int64_t)1 << 25;
    for (int64_t r0 = 0; r0 < rows; r0 += rows_per_launch) {
        const int64_t nr = std::min<int64_t>(rows - r0, rows_per_launch);
        const int8_t *xs = x + r0 * C;
        int8_t *os = out8 + r0 * C;
        const unsigned grid2 = (unsigned)((nr + 7) / 8);
        if (lut_old || iter > 6) shiftgelu_lut_kernel<<<(unsigned)((nr + 3) / 4), 256, 0, h->stream>>>(xs, nr, C, table, os);
        else if (iter == 1) shiftgelu_lut2_kernel<1><<<grid2, 256, 0, h->stream>>>(xs, nr, C, table, os);
        else if (iter == 2) shiftgelu_lut2_kernel<2><<<grid2, 256, 0, h->stream>>>(xs, nr, C, table, os);
        else if (iter == 3) shiftgelu_lut2_kernel<3><<<grid2, 256, 0, h->stream>>>(xs, nr, C, table, os);
        else if (iter == 4) shiftgelu_lut2_kernel<4><<<grid2, 256, 0, h->stream>>>(xs, nr, C, table, os);
        else shiftgelu_lut2_kernel<6><<<grid2, 256, 0, h->stream>>>(xs, nr, C, table, os);
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_layernorm(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale, const float *bias_int,
                   const float *sc, float *z) {
    CHECK_H(h);
    REQUIRE(h, x && bias_int && sc && z && rows > 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE(h, (C % 8) == 0, "C must be a multiple of 8");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, z, "z");
    REQUIRE_DISJOINT(h, x, (size_t)rows * C * 2, "x", z, (size_t)rows * C * 4, "z", OVL_IN);
    const size_t lds = (size_t)8 * C * sizeof(float);
    REQUIRE(h, lds <= 160 * 1024, "C too large for LDS staging");
    REQUIRE_LAUNCH(h, (rows + 7) / 8, 256, 8);
    if (int st = launch_dyn<layernorm_kernel<false>>(h, (unsigned)((rows + 7) / 8), 256, lds, x, rows, C, C, scale, bias_int, sc, nullptr, z)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// layernorm_reg_kernel<CC, S, MERGE> on `rows` rows (x, scale, bias_int, sc, dy_ch, out8 of the enclosing entry), and out of the entry
#define LNR_LAUNCH(CC, S, MERGE, row_stride, merge_R)                                                                     \
    do {                                                                                                                  \
        constexpr int rpb = (LNR_THREADS(S) / 64) * (64 / (4 * S));                                                       \
        REQUIRE_LAUNCH(h, (rows + rpb - 1) / rpb, LNR_THREADS(S), rpb);                                                   \
        layernorm_reg_kernel<CC, S, MERGE><<<(unsigned)((rows + rpb - 1) / rpb), LNR_THREADS(S), 0, h->stream>>>(        \
            x, rows, row_stride, scale, bias_int, sc, dy_ch, out8, merge_R);                                              \
        LAUNCH_CHECK(h);                                                                                                  \
        return IVIT_OK;                                                                                                   \
    } while (0)

int ivit_layernorm_requant(ivit_handle h, const int16_t *x, int64_t rows, int C, int64_t row_stride, float scale,
                           const float *bias_int, const float *sc, const ivit_dyadic *dy_ch, int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && bias_int && sc && dy_ch && out8 && rows > 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE(h, (C % 8) == 0 && (row_stride % 8) == 0 && row_stride >= C, "C, row_stride multiples of 8");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out8, "out8");
    REQUIRE_DISJOINT(h, x, span_bytes(rows, row_stride, C, 2), "x", out8, (size_t)rows * C, "out8", OVL_IN);
    {   // production form: the row in registers, 4 S lanes per row (ivit_layernorm.h)
#define LNR(CC, S) LNR_LAUNCH(CC, S, false, row_stride, 0)
        switch (C) {
            // lanes per row = 4 S (measured on DeiT-S b256: S = 1 23.2 us, S = 2 20.1, S = 4 20.2 — shorter per-wave instruction
            // chains and more waves per SIMD beat the cheaper quad-only reduction).  ivit_layernorm.h has the history of S = 1
            case 96: LNR(96, 2);        // Swin-T/S stage 0 (token-order sums use their own kernel)
            case 128: LNR(128, 2);      // Swin-B stage 0
            case 192: LNR(192, 2);      // DeiT-T, Swin stage 1
            case 256: LNR(256, 2);
            case 384: LNR(384, 2);      // DeiT-S, Swin stage 2, PatchMerging
            case 512: LNR(512, 4);
            case 768: LNR(768, 4);      // DeiT-B / ViT-B, Swin stage 3
            case 1024: LNR(1024, 4);    // ViT-L
            case 1536: LNR(1536, 4);    // Swin PatchMerging before stage 3
            default: break;
        }
#undef LNR
    }
    {   // other channel counts: 16 lanes per row, the row staged in LDS
        const size_t lds16 = (size_t)16 * (C + 16) * 4 + (size_t)C * 20;
        if (lds16 <= 150 * 1024) {
            long long riter = rows / (16LL * 6 * h->num_cu);
            riter = riter < 1 ? 1 : (riter > LN_RITER ? LN_RITER : riter);
            const long long per_block = 16 * riter;
            REQUIRE_LAUNCH(h, (rows + per_block - 1) / per_block, 256, per_block);
            const unsigned grid = (unsigned)((rows + per_block - 1) / per_block);
            if (int st = launch_dyn<layernorm16_kernel<0>>(h, grid, 256, lds16, x, rows, C, row_stride, scale, bias_int, sc, dy_ch, out8, (int)riter)) return st;
            LAUNCH_CHECK(h);
            return IVIT_OK;
        }
    }
    const size_t lds = (size_t)8 * C * sizeof(float);
    REQUIRE(h, lds <= 160 * 1024, "C too large for LDS staging");
    REQUIRE_LAUNCH(h, (rows + 7) / 8, 256, 8);
    if (int st = launch_dyn<layernorm_kernel<true>>(h, (unsigned)((rows + 7) / 8), 256, lds, x, rows, C, row_stride, scale, bias_int, sc, dy_ch, out8)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// PatchMerging's gather folded into the LayerNorm that follows it (swin_quant.py:336-349: the 2 x 2 gather, norm over 4C, qact1):
// x int16 [B, R, R, C] -> out8 int8 [B (R/2)^2, 4C].  Same integers as ivit_patch_merge_gather + ivit_layernorm_requant.
int ivit_patch_merge_layernorm_requant(ivit_handle h, const int16_t *x, int B, int R, int C, float scale, const float *bias_int,
                                       const float *sc, const ivit_dyadic *dy_ch, int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && bias_int && sc && dy_ch && out8 && B > 0 && R > 0 && (R % 2) == 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, out8, "out8");
    REQUIRE_DISJOINT(h, x, (size_t)B * R * R * C * 2, "x", out8, (size_t)B * R * R * C, "out8", OVL_IN);
    const long long rows = (long long)B * (R / 2) * (R / 2);
#define LNM(CC, S) LNR_LAUNCH(CC, S, true, 0, R)
    switch (4 * C) {
        case 384: LNM(384, 2);       // Swin-T/S: 96 -> 384
        case 512: LNM(512, 4);       // Swin-B: 128 -> 512
        case 768: LNM(768, 4);
        case 1024: LNM(1024, 4);
        case 1536: LNM(1536, 4);
        default: break;
    }
#undef LNM
#undef LNR_LAUNCH
    snprintf(h->err, sizeof(h->err), "%s: built for C = 96, 128, 192, 256, 384 (use ivit_patch_merge_gather + ivit_layernorm_requant)", __func__);
    return IVIT_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------- Swin-specific operators
int ivit_shiftmax_masked(ivit_handle h, const int8_t *x, int64_t rows, int n, int ld_in, float scale, int out_bits,
                         const float *mask, int nW, int H, uint16_t *out, int ld_out) {
    CHECK_H(h);
    REQUIRE(h, x && out && rows > 0 && n > 0 && ld_in >= n && ld_out >= n && scale > 0.f, "bad arguments");
    REQUIRE(h, out_bits == 8 || out_bits == 16, "out_bits must be 8 or 16");
    REQUIRE_DISJOINT(h, x, span_bytes(rows, ld_in, n, 1), "x", out, span_bytes(rows, ld_out, n, 2), "out", OVL_IN);
    REQUIRE(h, mask == nullptr || (nW > 0 && H > 0), "mask needs nW, H");
    const size_t lds = (size_t)4 * n * sizeof(float);
    REQUIRE(h, lds <= 160 * 1024, "row too long for LDS staging");
    REQUIRE_LAUNCH(h, (rows + 3) / 4, 256, 4);
    if (int st = launch_dyn<shiftmax_masked_kernel>(h, (unsigned)((rows + 3) / 4), 256, lds, x, rows, n, ld_in, scale, out_bits, mask,
                                                    nW > 0 ? nW : 1, H > 0 ? H : 1, out, ld_out))
        return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_requant_i32_bcast(ivit_handle h, const int32_t *z, ivit_dyadic dy, const int32_t *z_id, int64_t id_period,
                           ivit_dyadic dy_id, int bits, void *out, int64_t total) {
    CHECK_H(h);
    REQUIRE(h, z && z_id && out && total > 0 && id_period > 0, "bad arguments");
    REQUIRE(h, bits == 8 || bits == 16, "bits must be 8 or 16");
    REQUIRE_DISJOINT(h, z, (size_t)total * 4, "z", out, (size_t)total * (bits / 8), "out", OVL_IN);
    const int g = grid_for(h, total, 256 * 4);
    if (bits == 8) requant_bcast_kernel<8><<<g, 256, 0, h->stream>>>(z, dy, z_id, id_period, dy_id, out, total);
    else requant_bcast_kernel<16><<<g, 256, 0, h->stream>>>(z, dy, z_id, id_period, dy_id, out, total);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_avgpool_requant(ivit_handle h, const int8_t *x, int B, int L, int C, ivit_dyadic dy, int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && out8 && B > 0 && L > 0 && C > 0, "bad arguments");
    REQUIRE(h, (L & 1) == 1, "token count must be odd (no rounding ties; see kernel comment)");
    REQUIRE_DISJOINT(h, x, (size_t)B * L * C, "x", out8, (size_t)B * C, "out8", OVL_IN);
    avgpool_requant_kernel<<<(unsigned)((B * C + 255) / 256), 256, 0, h->stream>>>(x, B, L, C, 0.f, dy, out8);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_avgpool_requant_scaled(ivit_handle h, const int8_t *x, int B, int L, int C, float scale, ivit_dyadic dy,
                                int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && out8 && B > 0 && L > 0 && C > 0 && scale > 0.f, "bad arguments");
    REQUIRE_DISJOINT(h, x, (size_t)B * L * C, "x", out8, (size_t)B * C, "out8", OVL_IN);
    avgpool_requant_kernel<<<(unsigned)((B * C + 255) / 256), 256, 0, h->stream>>>(x, B, L, C, scale, dy, out8);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// LDS bytes of layernorm_tokenorder_kernel at C channels; of layernorm_tokenorder8_kernel (C = 96 / 128), and its grid
static inline size_t lnt_lds(int C) { return ((size_t)LNT_ROWS * (C + 1) + 3 * (size_t)C + 2 * LNT_ROWS + 2) * sizeof(float) + (size_t)C * sizeof(double); }
static inline size_t lnt8_lds(int C) { return ((size_t)LNT8_ROWS * (C + 1) + C + 2 * LNT8_ROWS) * sizeof(float); }
static inline unsigned lnt8_grid(int64_t rows) { return (unsigned)((rows + LNT8_ROWS - 1) / LNT8_ROWS); }

int ivit_layernorm_tokenorder_requant(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale,
                                      const float *bias_int, const float *sc, const ivit_dyadic *dy,
                                      int tokens_per_image, int8_t *out8) {
    CHECK_H(h);
    REQUIRE(h, x && bias_int && sc && dy && out8 && rows > 0 && C > 0 && scale > 0.f && tokens_per_image > 0, "bad arguments");
    REQUIRE_DISJOINT(h, x, (size_t)rows * C * 2, "x", out8, (size_t)rows * C, "out8", OVL_IN);
    const size_t lds = lnt_lds(C);
    REQUIRE(h, lds <= 160 * 1024, "C too large for LDS staging");
    REQUIRE_LAUNCH(h, (rows + LNT_ROWS - 1) / LNT_ROWS, 256, LNT_ROWS);      // (the 96-row form of C = 96 / 128 has fewer, no larger blocks)
    int st;
    if (C == 96 || C == 128) {          // Swin-T/S and Swin-B stage 0
        REQUIRE(h, (((uintptr_t)x | (uintptr_t)out8 | (uintptr_t)bias_int | (uintptr_t)sc) & 15) == 0,
                "C = 96 / 128: x, out, bias_int, sc must be 16-byte aligned (vector loads)");
        st = with_width(C, [&](auto W) {
            return launch_dyn<layernorm_tokenorder8_kernel<1, W(), int16_t>>(h, lnt8_grid(rows), W() / 8 * 16, lnt8_lds(C), x, rows, scale, bias_int, sc, dy,
                                                                             tokens_per_image, out8, ivit_dyadic{0.0, 0.0});
        });
    } else {
        st = launch_dyn<layernorm_tokenorder_kernel<1, 0>>(h, (unsigned)((rows + LNT_ROWS - 1) / LNT_ROWS), 256, lds, x, rows, C, scale, bias_int, sc, dy,
                                                           tokens_per_image, out8, ivit_dyadic{0.0, 0.0});
    }
    if (st) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_patch_norm_tokenorder(ivit_handle h, const int8_t *x8, int64_t rows, int C, float scale, const float *bias_int,
                               const float *sc, const ivit_dyadic *dy_ch, ivit_dyadic dy2, int tokens_per_image,
                               int16_t *out16) {
    CHECK_H(h);
    REQUIRE(h, x8 && bias_int && sc && dy_ch && out16 && rows > 0 && C > 0 && scale > 0.f && tokens_per_image > 0, "bad arguments");
    REQUIRE_DISJOINT(h, x8, (size_t)rows * C, "x8", out16, (size_t)rows * C * 2, "out16", OVL_IN);
    const size_t lds = lnt_lds(C);
    REQUIRE(h, lds <= 160 * 1024, "C too large for LDS staging");
    REQUIRE_LAUNCH(h, (rows + LNT_ROWS - 1) / LNT_ROWS, 256, LNT_ROWS);      // (the 96-row form of C = 96 / 128 has fewer, no larger blocks)
    int st;
    if (C == 96 || C == 128) {
        REQUIRE(h, (((uintptr_t)x8 | (uintptr_t)out16 | (uintptr_t)bias_int | (uintptr_t)sc) & 15) == 0,
                "C = 96 / 128: x, out, bias_int, sc must be 16-byte aligned (vector loads)");
        st = with_width(C, [&](auto W) {
            return launch_dyn<layernorm_tokenorder8_kernel<2, W(), int8_t>>(h, lnt8_grid(rows), W() / 8 * 16, lnt8_lds(C), x8, rows, scale, bias_int, sc, dy_ch,
                                                                            tokens_per_image, out16, dy2);
        });
    } else {
        st = launch_dyn<layernorm_tokenorder_kernel<2, 0, int8_t>>(h, (unsigned)((rows + LNT_ROWS - 1) / LNT_ROWS), 256, lds, x8, rows, C, scale, bias_int, sc,
                                                                   dy_ch, tokens_per_image, out16, dy2);
    }
    if (st) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_layernorm_tokenorder(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale,
                              const float *bias_int, const float *sc, int tokens_per_image, float *z) {
    CHECK_H(h);
    REQUIRE(h, x && bias_int && sc && z && rows > 0 && C > 0 && scale > 0.f && tokens_per_image > 0, "bad arguments");
    REQUIRE_DISJOINT(h, x, (size_t)rows * C * 2, "x", z, (size_t)rows * C * 4, "z", OVL_IN);
    const size_t lds = lnt_lds(C);
    REQUIRE(h, lds <= 160 * 1024, "C too large for LDS staging");
    REQUIRE_LAUNCH(h, (rows + LNT_ROWS - 1) / LNT_ROWS, 256, LNT_ROWS);      // (the 96-row form of C = 96 / 128 has fewer, no larger blocks)
    if (int st = launch_dyn<layernorm_tokenorder_kernel<0, 0>>(h, (unsigned)((rows + LNT_ROWS - 1) / LNT_ROWS), 256, lds, x, rows, C, scale, bias_int, sc,
                                                               nullptr, tokens_per_image, z, ivit_dyadic{0.0, 0.0}))
        return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_debug_div(ivit_handle h, const float *n, const float *d, float *q_ieee, float *q_lean, int64_t count) {
    CHECK_H(h);
    REQUIRE(h, n && d && q_ieee && q_lean && count > 0, "bad arguments");
    REQUIRE_LAUNCH(h, (count + 255) / 256, 256, 256);
    debug_div_kernel<<<(unsigned)((count + 255) / 256), 256, 0, h->stream>>>(n, d, q_ieee, q_lean, count);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_debug_requotient(ivit_handle h, const float *q, const float *d, float *r_ieee, float *r_markstein, int64_t count) {
    CHECK_H(h);
    REQUIRE(h, q && d && r_ieee && r_markstein && count > 0, "bad arguments");
    REQUIRE_LAUNCH(h, (count + 255) / 256, 256, 256);
    debug_requotient_kernel<<<(unsigned)((count + 255) / 256), 256, 0, h->stream>>>(q, d, r_ieee, r_markstein, count);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_im2col_patch(ivit_handle h, const int8_t *img, int B, int Cin, int H, int W, int P, int8_t *rows) {
    CHECK_H(h);
    REQUIRE(h, img && rows && B > 0 && Cin > 0 && P > 0, "bad arguments");
    REQUIRE(h, (H % P) == 0 && (W % P) == 0 && (P % 4) == 0 && (W % 4) == 0, "H,W multiples of P; P,W multiples of 4");
    REQUIRE_A16(h, img, "img");
    REQUIRE_A16(h, rows, "rows");
    REQUIRE_DISJOINT(h, img, (size_t)B * Cin * H * W, "img", rows, (size_t)B * Cin * H * W, "rows", OVL_IN);
    const size_t lds = (size_t)Cin * P * W;
    REQUIRE(h, lds <= 64 * 1024, "patch strip too large for LDS staging");
    if (P == 16 && Cin == 3 && (W % 16) == 0 && B <= 65535)
        im2col_patch16_kernel<3><<<dim3((unsigned)(H / P), (unsigned)B), 256, lds, h->stream>>>(img, H, W, rows);
    else {
        REQUIRE_LAUNCH(h, (long long)B * (H / P), 256, 1);
        im2col_patch_kernel<<<(unsigned)((long long)B * (H / P)), 256, lds, h->stream>>>(img, B, Cin, H, W, P, rows);
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_embed_finish(ivit_handle h, const int16_t *patch16, const int32_t *z_cls, const int16_t *pos,
                      ivit_dyadic dy_x, ivit_dyadic dy_pos, int16_t *x16, int B, int T, int D) {
    CHECK_H(h);
    REQUIRE(h, patch16 && z_cls && pos && x16 && B > 0 && T > 1 && D > 0 && (D % 8) == 0, "bad arguments (D must be a multiple of 8)");
    REQUIRE(h, (long long)T * D / 8 < (1 << 22) && B <= 65535, "T * D / 8 < 2^22, B < 2^16");
    REQUIRE_A16(h, patch16, "patch16");
    REQUIRE_A16(h, x16, "x16");
    REQUIRE_DISJOINT(h, patch16, (size_t)B * (T - 1) * D * 2, "patch16", x16, (size_t)B * T * D * 2, "x16", OVL_IN);
    const int fast = rq_fast2(dy_x, dy_pos);
    embed_finish_kernel<<<dim3((unsigned)((T * (D / 8) + 255) / 256), (unsigned)B), 256, 0, h->stream>>>(
        patch16, z_cls, pos, dy_x, dy_pos, x16, T, D, 1.0f / (float)(D / 8), fast);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_patch_embed(ivit_handle h, const int8_t *images, int B, int C, int H, int W, int P, const int8_t *w, const int32_t *bias,
                     const ivit_dyadic *dy_ch, const int32_t *z_cls, const int16_t *pos, ivit_dyadic dy_x, ivit_dyadic dy_pos,
                     int16_t *x16, int D) {
    CHECK_H(h);
    REQUIRE(h, images && w && dy_ch && z_cls && pos && x16 && B > 0 && C > 0 && H > 0 && W > 0 && P > 0 && D > 0, "bad arguments");
    REQUIRE_A16(h, images, "images");
    REQUIRE_A16(h, x16, "x16");
    const int gh = H / P, gw = W / P, np = gh * gw, K = C * P * P, T = np + 1;
    REQUIRE_DISJOINT(h, images, (size_t)B * C * H * W, "images", x16, (size_t)B * T * D * 2, "x16", OVL_IN);
    const bool fast = rq_fast2(dy_x, dy_pos);
    GemmArgs a = linear_args(images, w, bias, B * np, D, K);
    if (P != 16 || H % 16 || W % 16 || (D % 8) != 0 || (K % 64) != 0 || !fast || !use_gemm2(a) || (long long)B * np >= (1ll << 30) ||
        (long long)T * D / 8 >= (1 << 22) || B > 65535) {
        snprintf(h->err, sizeof(h->err), "%s: built for 16 x 16 patches, K %% 64 == 0, both multipliers in the fast range", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    // class-token rows, then every patch row from the GEMM's epilogue: QuantConv2d -> QuantAct(16) -> + pos -> QuantAct(16) (vit_quant.py:255-265)
    embed_finish_kernel<<<dim3((unsigned)((D / 8 + 255) / 256), (unsigned)B), 256, 0, h->stream>>>(nullptr, z_cls, pos, dy_x, dy_pos, x16, T, D,
                                                                                                  1.0f / (float)(D / 8), 1, 1);
    LAUNCH_CHECK(h);
    a.out = x16; a.dy_ch = dy_ch; a.dy_main = dy_x; a.dy_res = dy_pos; a.residual = pos;
    a.img = images; a.img_C = C; a.img_H = H; a.img_W = W; a.pe_gw = gw; a.pe_P = np;
    a.tiles_n = (a.N + G2_BN - 1) / G2_BN;
    const long long t128 = (long long)((a.M + 127) / 128) * a.tiles_n;
    gemm_glds_kernel<EPI_RQ16_CH_RES, 128, true><<<dim3((unsigned)t128), 256, 0, h->stream>>>(a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

}  // extern "C"

extern "C" {

// window 12 (ivit_swin12.h window_attention12_kernel): arithmetic Shiftmax only
static int window_attention12_launch(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a, const int16_t *relb,
                                     float s_softmax, bool tables, ivit_dyadic dy_pv, int8_t *ctx, int B, int R, int shift,
                                     int heads, int dh) {
    if (tables) {
        snprintf(h->err, sizeof(h->err), "window_attention: the Shiftmax-table form is built for window 7 only; "
                                         "use ivit_window_attention_fused at window 12");
        return IVIT_ERR_UNSUPPORTED;
    }
    if (dh != 32 || (R % 12) != 0) {
        snprintf(h->err, sizeof(h->err), "window_attention: window 12 is built for head dim 32 and R %% 12 == 0");
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE(h, shift >= 0 && shift < 12 && s_softmax > 0.f, "bad shift / scale");
    REQUIRE(h, fabs(dy_qk.m * dy_qk.r) < 2048.0 && fabs(dy_pv.m * dy_pv.r) < 1024.0, "requant factor out of range");
    REQUIRE(h, ((uintptr_t)relb & 15) == 0, "relb must be 16-byte aligned (staged in 16-byte pieces)");
    WinAttn12Args a;
    memset(&a, 0, sizeof(a));
    a.qkv = qkv; a.ctx = ctx; a.relb = relb; a.B = B; a.R = R; a.shift = shift; a.heads = heads;
    a.dy_qk = dy_qk; a.dy_a = dy_a; a.dy_pv = dy_pv; a.s = s_softmax;
    const long long nwin = (long long)B * (R / 12) * (R / 12);
    // windows per block: the slab (41.5 KB) is staged once per block, so as many as keep >= 3 blocks per resident
    // slot (2 per CU of the handle's CU share, ivit_set_cu_share), at most 8
    const long long slots = 2LL * persistent_cus(h);
    int wpb = 8;
    while (wpb > 1 && ((nwin + wpb - 1) / wpb) * heads < 3 * slots) wpb >>= 1;
    a.wpb = wpb;
    const long long groups = (nwin + wpb - 1) / wpb;      // grid: whole groups of 8 window groups (see the kernel)
    if (int st = launch_dyn<window_attention12_kernel<12>>(h, (unsigned)(((groups + 7) / 8) * 8 * heads), WA12_THREADS, WA12_SMEM, a)) return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

static int window_attention_impl(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a,
                                 const int16_t *relb, float s_softmax, const uint16_t *aq, const float *et, const uint8_t *cls,
                                 int nc, int t_count, int dmin, ivit_dyadic dy_pv, int8_t *ctx, int B, int R,
                                 int window, int shift, int heads, int dh) {
    CHECK_H(h);
    REQUIRE(h, qkv && relb && ctx && B > 0 && R > 0 && heads > 0, "bad arguments");
    REQUIRE_A16(h, qkv, "qkv");
    REQUIRE_A16(h, ctx, "ctx");
    if (dh > 0) REQUIRE_DISJOINT(h, qkv, (size_t)B * R * R * 3 * heads * dh, "qkv", ctx, (size_t)B * R * R * heads * dh, "ctx", OVL_IN);
    if (window == 12) return window_attention12_launch(h, qkv, dy_qk, dy_a, relb, s_softmax, aq != nullptr, dy_pv, ctx, B, R,
                                                       shift, heads, dh);
    if (window != 7 || dh != 32 || (R % 7) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: built for windows 7 and 12, head dim 32, R %% window == 0", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE(h, shift >= 0 && shift < 7 && s_softmax > 0.f, "bad shift / scale");
    // magic-number rounding needs |z*c| < 2^31 with |q.k| <= 2^19 and |sum P*v| <= 2^20
    REQUIRE(h, fabs(dy_qk.m * dy_qk.r) < 2048.0 && fabs(dy_pv.m * dy_pv.r) < 1024.0, "requant factor out of range");
    WinAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.qkv = qkv; a.ctx = ctx; a.relb = relb; a.B = B; a.R = R; a.shift = shift; a.heads = heads;
    a.dy_qk = dy_qk; a.dy_a = dy_a; a.dy_pv = dy_pv; a.s = s_softmax;
    a.units = (long long)B * (R / 7) * (R / 7) * heads;
    a.wpw = 1;
    const long long nwin = (long long)B * (R / 7) * (R / 7);
    if (aq) {
        REQUIRE(h, et && cls && nc >= 1 && nc <= 64 && t_count >= 1 && t_count <= 16384 && dmin <= 0 && dmin >= -255,
                "bad Shiftmax tables");
        REQUIRE(h, (((uintptr_t)aq | (uintptr_t)et) & 15) == 0 && ((uintptr_t)cls & 3) == 0,
                "Shiftmax tables: exp_aq and exp_t must be 16-byte aligned, exp_cls 4-byte aligned (copied in 16-byte pieces)");
        a.aq = aq; a.et = et; a.cls = cls; a.nc = nc; a.t_count = t_count; a.dmin = dmin;
        // windows per wavefront: as many as keep >= 3 workgroups per resident slot (2 per CU), at most 4
        const long long slots = 2LL * h->num_cu;
        int wpw = 4;
        while (wpw > 1 && ((nwin + 8LL * wpw - 1) / (8LL * wpw)) * heads < 3 * slots) wpw >>= 1;
        a.wpw = wpw;
        const size_t lds = WA_FIXED(8) + (size_t)((t_count + 3) & ~3) * 4 + (size_t)nc * 512 + 256;
        const long long groups = (nwin + 8LL * wpw - 1) / (8LL * wpw);      // grid: whole groups of 8 window groups (see the kernel)
        if (int st = launch_dyn<window_attention_kernel<true>>(h, (unsigned)(((groups + 7) / 8) * 8 * heads), 512, lds, a)) return st;
    } else {
        const long long groups = (nwin + 3) / 4;
        window_attention_kernel<false><<<dim3((unsigned)(((groups + 7) / 8) * 8 * heads)), 256, WA_FIXED(4), h->stream>>>(a);
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_window_attention_fused(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a,
                                const int16_t *relb, float s_softmax, ivit_dyadic dy_pv, int8_t *ctx, int B, int R,
                                int window, int shift, int heads, int dh) {
    return window_attention_impl(h, qkv, dy_qk, dy_a, relb, s_softmax, nullptr, nullptr, nullptr, 0, 0, 0, dy_pv, ctx, B, R,
                                 window, shift, heads, dh);
}

int ivit_window_attention_fused_lut(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a,
                                    const int16_t *relb, float s_softmax, const uint16_t *exp_aq, const float *exp_t,
                                    const uint8_t *exp_cls, int nclass, int t_count, int dmin, ivit_dyadic dy_pv,
                                    int8_t *ctx, int B, int R, int window, int shift, int heads, int dh) {
    if (h && !(exp_aq && exp_t && exp_cls)) { snprintf(h->err, sizeof(h->err), "ivit_window_attention_fused_lut: null table"); return IVIT_ERR_INVALID; }
    return window_attention_impl(h, qkv, dy_qk, dy_a, relb, s_softmax, exp_aq, exp_t, exp_cls, nclass, t_count, dmin, dy_pv, ctx,
                                 B, R, window, shift, heads, dh);
}

int ivit_mlp_fused(ivit_handle h, const int8_t *x, const int8_t *w1, const int32_t *b1, const ivit_dyadic *dy1,
                   const int8_t *gelu_table, const int8_t *w2, const int32_t *b2, const ivit_dyadic *dy2,
                   ivit_dyadic dy_main, ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int64_t M, int C,
                   int hidden) {
    CHECK_H(h);
    REQUIRE(h, x && w1 && dy1 && gelu_table && w2 && dy2 && residual && out && M > 0, "bad arguments");
    if ((C == Mlp128Geo::C && hidden == Mlp128Geo::HD) || (C == MF_C && hidden == MF_HD)) {
        // judged at the two widths the entry is built for: at any other (C, hidden) it addresses nothing, and the extents of a shape it
        // refuses as unsupported describe no array.  residual == out refused: all three kernels fetch the identity of rows past M - 1
        // of a tile from row M - 1
        REQUIRE_DISJOINT(h, x, (size_t)M * C, "x", out, (size_t)M * C * 2, "out", OVL_IN);
        REQUIRE_DISJOINT(h, residual, (size_t)M * C * 2, "residual", out, (size_t)M * C * 2, "out", OVL_IN);
    }
    if (C == Mlp128Geo::C && hidden == Mlp128Geo::HD)
        return mlp128_launch(h, x, w1, b1, dy1, gelu_table, w2, b2, dy2, dy_main, dy_res, residual, out, M);
    if (C != MF_C || hidden != MF_HD) {
        snprintf(h->err, sizeof(h->err), "%s: built for C = 96, hidden = 384 (weights resident in LDS) and C = 128, hidden = 512 (weights streamed from L2)",
                 __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, residual, "residual");
    REQUIRE_A16(h, out, "out");
    MlpFusedArgs a;
    a.x = x; a.w1 = w1; a.b1 = b1; a.dy1 = dy1; a.tab = gelu_table; a.w2 = w2; a.b2 = b2; a.dy2 = dy2;
    a.dy_main = dy_main; a.dy_res = dy_res; a.residual = residual; a.out = out; a.M = M;
    const long long ntiles = (M + MF_BM - 1) / MF_BM;
    const unsigned grid = (unsigned)(ntiles < h->num_cu ? ntiles : h->num_cu);
    // role-split form (ivit_swin_mlp_rs.h: producers on fc1 of tile i + 1 beside consumers on ShiftGELU / fc2 of tile i) when a
    // workgroup has at least two tiles to overlap; the phase-by-phase kernel otherwise
    if (int st = ntiles >= 2 * (long long)grid ? launch_dyn<swin_mlp_rs_kernel>(h, grid, SR_THREADS, SR_SMEM, a)
                                               : launch_dyn<swin_mlp_fused_kernel>(h, grid, MF_THREADS, MF_SMEM, a))
        return st;
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_patch_merge_gather(ivit_handle h, const void *x, int in_bits, int B, int R, int C, int16_t *out) {
    CHECK_H(h);
    REQUIRE(h, x && out && B > 0 && R > 0 && (R % 2) == 0 && C > 0 && (C % 8) == 0, "bad arguments (C must be a multiple of 8)");
    REQUIRE(h, in_bits == 8 || in_bits == 16, "in_bits must be 8 or 16");
    if (in_bits == 16) REQUIRE_A16(h, x, "x");
    else REQUIRE_ALIGNED(h, x, "x", 8);
    REQUIRE_A16(h, out, "out");
    REQUIRE_DISJOINT(h, x, (size_t)B * R * R * C * (in_bits / 8), "x", out, (size_t)B * R * R * C * 2, "out", OVL_IN);
    const long long total = (long long)B * R * R * C / 8;
    if (in_bits == 8) patch_merge_gather_kernel<int8_t><<<grid_for(h, total, 1024), 256, 0, h->stream>>>((const int8_t *)x, B, R, C, out);
    else patch_merge_gather_kernel<int16_t><<<grid_for(h, total, 1024), 256, 0, h->stream>>>((const int16_t *)x, B, R, C, out);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_widen_i8_i16(ivit_handle h, const int8_t *x, int16_t *out, int64_t n) {
    CHECK_H(h);
    REQUIRE(h, x && out && n >= 0, "bad arguments");
    REQUIRE_DISJOINT(h, x, (size_t)n, "x", out, (size_t)n * 2, "out", OVL_IN);
    if (n == 0) return IVIT_OK;
    widen_i8_i16_kernel<<<grid_for(h, n, 1024), 256, 0, h->stream>>>(x, out, n);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_logits_topk(ivit_handle h, const int32_t *logits, const float *scale, int batch, int num_classes, int k, int32_t *idx,
                     float *val) {
    CHECK_H(h);
    REQUIRE(h, logits && scale && idx && batch >= 0 && num_classes >= 1, "bad arguments");
    REQUIRE(h, k >= 1 && k <= TOPK_MAX_K && k <= num_classes, "k must be in 1 .. min(16, num_classes)");
    {
        const size_t nin = (size_t)batch * num_classes * 4, nout = (size_t)batch * k * 4;
        REQUIRE_DISJOINT(h, logits, nin, "logits", idx, nout, "idx", OVL_IN);
        REQUIRE_DISJOINT(h, logits, nin, "logits", val, nout, "val", OVL_IN);
        REQUIRE_DISJOINT(h, idx, nout, "idx", val, nout, "val", OVL_OUT);
    }
    if (batch == 0) return IVIT_OK;
    REQUIRE_LAUNCH(h, (batch + 3ll) / 4, 256, 4);
    const unsigned grid = (unsigned)((batch + 3ll) / 4);        // one wavefront per image; 64-bit sum: no overflow near INT_MAX
    if (num_classes <= TOPK_REG_CLASSES) logits_topk_kernel<true><<<grid, 256, 0, h->stream>>>(logits, scale, batch, num_classes, k, idx, val);
    else logits_topk_kernel<false><<<grid, 256, 0, h->stream>>>(logits, scale, batch, num_classes, k, idx, val);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

int ivit_logits_score(ivit_handle h, const int32_t *logits, const float *scale, const int64_t *labels, int batch, int num_classes,
                      int32_t *rank, double *nll) {
    CHECK_H(h);
    REQUIRE(h, logits && scale && labels && batch >= 0 && num_classes >= 1, "bad arguments");
    REQUIRE(h, rank || nll, "rank and nll are both null");
    if (batch == 0) return IVIT_OK;
    REQUIRE_LAUNCH(h, (batch + 3ll) / 4, 256, 4);
    const unsigned grid = (unsigned)((batch + 3ll) / 4);        // one wavefront per image, as ivit_logits_topk
    const long long *lab = (const long long *)labels;
    if (num_classes <= TOPK_REG_CLASSES) logits_score_kernel<true><<<grid, 256, 0, h->stream>>>(logits, scale, lab, batch, num_classes, rank, nll);
    else logits_score_kernel<false><<<grid, 256, 0, h->stream>>>(logits, scale, lab, batch, num_classes, rank, nll);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

}  // extern "C"

// the argument rules the features entries share (ivit_model.h asks here before its slices are launched: `out` is its feat32 and may be absent)
static int features_args_ok(ivit_handle h, const char *fn, const int8_t *feat8, int dim, float scale, int mode, const float *out, bool feat32) {
    const char *bad = nullptr;
    if (!feat8) bad = "feat8 is null";
    else if (mode != IVIT_FEATURES_DEQUANT && mode != IVIT_FEATURES_UNIT) bad = "mode must be IVIT_FEATURES_DEQUANT or IVIT_FEATURES_UNIT";
    else if (out && !(scale > 0.f && scale <= FLT_MAX)) bad = "scale must be finite and positive";
    else if (dim < 1) bad = "dim must be positive";
    else if ((uintptr_t)feat8 & 15) bad = "feat8 must be 16-byte aligned";
    else if ((uintptr_t)out & 15) bad = feat32 ? "feat32 must be 16-byte aligned" : "out must be 16-byte aligned";
    if (bad) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    if ((dim % 16) != 0 || dim > FEATURES_MAX_DIM) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 16 and at most %d", fn, FEATURES_MAX_DIM);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

extern "C" int ivit_features_f32(ivit_handle h, const int8_t *feat8, int batch, int dim, float scale, int mode, float *out) {
    CHECK_H(h);
    REQUIRE(h, out && batch >= 0, "out is null or batch is negative");
    if (const int rc = features_args_ok(h, __func__, feat8, dim, scale, mode, out, false)) return rc;
    if (batch == 0) return IVIT_OK;
    REQUIRE_LAUNCH(h, (batch + 3ll) / 4, 256, 4);
    const unsigned grid = (unsigned)((batch + 3ll) / 4);        // one wavefront per row
    if (mode == IVIT_FEATURES_UNIT) features_f32_kernel<true><<<grid, 256, 0, h->stream>>>(feat8, batch, dim, scale, out);
    else features_f32_kernel<false><<<grid, 256, 0, h->stream>>>(feat8, batch, dim, scale, out);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- class-token attention maps (include/ivit_attnmap.h)
// the shape rules of ivit_attention_cls_probs (ivit_model.h asks here for its model, before its slices are launched)
static int attnmap_shape_ok(ivit_handle h, const char *fn, int T, int dh) {
    if ((dh % 16) != 0 || dh > ATTNMAP_MAX_DH || T > ATTNMAP_MAX_T) {
        snprintf(h->err, sizeof(h->err), "%s: dh must be a multiple of 16 and at most %d, T at most %d", fn, ATTNMAP_MAX_DH, ATTNMAP_MAX_T);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

extern "C" int ivit_attention_cls_probs(ivit_handle h, const int8_t *q, const int8_t *k, ivit_dyadic dy_qk, float s_softmax, uint16_t *p_cls, int B,
                                        int H, int T, int dh) {
    CHECK_H(h);
    REQUIRE(h, q && k && p_cls && B > 0 && H > 0 && T > 0 && dh > 0, "q, k or p_cls is null, or B, H, T, dh is not positive");
    REQUIRE(h, s_softmax > 0.f && s_softmax <= FLT_MAX, "s_softmax must be finite and positive");
    REQUIRE_A16(h, q, "q");
    REQUIRE_A16(h, k, "k");
    REQUIRE_ALIGNED(h, p_cls, "p_cls", 2);
    const size_t nqk = (size_t)B * H * T * dh, np = (size_t)B * H * T * 2;
    REQUIRE_DISJOINT(h, q, nqk, "q", p_cls, np, "p_cls", OVL_IN);
    REQUIRE_DISJOINT(h, k, nqk, "k", p_cls, np, "p_cls", OVL_IN);
    if (const int rc = attnmap_shape_ok(h, __func__, T, dh)) return rc;
    const long long BH = (long long)B * H;
    REQUIRE(h, BH <= 0x7fffffffLL, "B * H does not fit an int");
    REQUIRE_LAUNCH(h, (BH + 3) / 4, 256, 4);
    const size_t lds = (size_t)4 * T * sizeof(float);            // at most 16 KB
    attn_cls_probs_kernel<<<(unsigned)((BH + 3) / 4), 256, lds, h->stream>>>(q, k, dy_qk.m * dy_qk.r, s_softmax, p_cls, (int)BH, T, dh);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// the argument rules of the fp32 map (ivit_model.h asks here too: `out` is its map32 and may be absent there)
static int attnmap_map_args_ok(ivit_handle h, const char *fn, const uint16_t *p_cls, const char *p_name, long long rows, int H, int T, int mode,
                               const float *out, const char *out_name) {
    char msg[96] = "";
    if (!p_cls) snprintf(msg, sizeof(msg), "%s is null", p_name);
    else if (rows < 0 || H < 1 || T < 1) snprintf(msg, sizeof(msg), "rows is negative, or H or T is not positive");
    else if (mode != IVIT_ATTNMAP_HEADS && mode != IVIT_ATTNMAP_MEAN) snprintf(msg, sizeof(msg), "mode must be IVIT_ATTNMAP_HEADS or IVIT_ATTNMAP_MEAN");
    else if ((uintptr_t)p_cls & 1) snprintf(msg, sizeof(msg), "%s must be 2-byte aligned", p_name);
    else if ((uintptr_t)out & 3) snprintf(msg, sizeof(msg), "%s must be 4-byte aligned", out_name);
    if (msg[0]) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, msg); return IVIT_ERR_INVALID; }
    return IVIT_OK;
}
static inline size_t attnmap_map_bytes(long long rows, int H, int T, int mode) {
    return (size_t)rows * (mode == IVIT_ATTNMAP_MEAN ? 1 : H) * (size_t)(T - 1) * 4;
}

extern "C" int ivit_attention_map_f32(ivit_handle h, const uint16_t *p_cls, int64_t rows, int H, int T, int mode, float *out) {
    CHECK_H(h);
    REQUIRE(h, out, "out is null");
    if (const int rc = attnmap_map_args_ok(h, __func__, p_cls, "p_cls", rows, H, T, mode, out, "out")) return rc;
    REQUIRE_DISJOINT(h, p_cls, (size_t)rows * H * T * 2, "p_cls", out, attnmap_map_bytes(rows, H, T, mode), "out", OVL_IN);
    if (H > ATTNMAP_MAX_H || T > ATTNMAP_MAX_T) {
        snprintf(h->err, sizeof(h->err), "%s: H must be at most %d and T at most %d", __func__, ATTNMAP_MAX_H, ATTNMAP_MAX_T);
        return IVIT_ERR_UNSUPPORTED;
    }
    const long long total = (long long)rows * (mode == IVIT_ATTNMAP_MEAN ? 1 : H) * (T - 1);
    if (total == 0) return IVIT_OK;
    REQUIRE_LAUNCH(h, (total + 255) / 256, 256, 256);
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (mode == IVIT_ATTNMAP_MEAN) attn_map_f32_kernel<true><<<grid, 256, 0, h->stream>>>(p_cls, (long long)rows, H, T, out);
    else attn_map_f32_kernel<false><<<grid, 256, 0, h->stream>>>(p_cls, (long long)rows, H, T, out);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- class-activation maps of a Swin (include/ivit_classmap.h)
// the argument rules of ivit_class_map (ivit_model.h asks here for its model and the caller's arrays, before its slices are launched):
// pointers, counts, alignment, the five overlapping pairs, then the width
static int classmap_args_ok(ivit_handle h, const char *fn, const int8_t *tok8, const int8_t *head_w, const int32_t *idx, int batch, int L, int C,
                            int num_classes, int k, const float *class_scale, const int32_t *cam32, const float *map32) {
    const char *bad = nullptr;
    if (!tok8 || !head_w || !idx || !cam32) bad = "tok8, head_w, idx or cam32 is null";
    else if (batch < 1 || L < 1 || C < 1 || num_classes < 1) bad = "batch, L, C or num_classes is not positive";
    else if (k < 1 || k > CLASSMAP_MAX_K) bad = "k must be in 1 .. 16";
    else if (!class_scale != !map32) bad = "class_scale and map32 must both be null or both be set";
    else if ((uintptr_t)tok8 & 15) bad = "tok8 must be 16-byte aligned";
    else if ((uintptr_t)head_w & 15) bad = "head_w must be 16-byte aligned";
    else if ((uintptr_t)idx & 3) bad = "idx must be 4-byte aligned";
    else if ((uintptr_t)class_scale & 3) bad = "class_scale must be 4-byte aligned";
    else if ((uintptr_t)cam32 & 3) bad = "cam32 must be 4-byte aligned";
    else if ((uintptr_t)map32 & 3) bad = "map32 must be 4-byte aligned";
    else if ((long long)batch * k > 0x7fffffffLL) bad = "batch * k does not fit an int";
    if (bad) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    const size_t ntok = (size_t)batch * L * C, nidx = (size_t)batch * k * 4, nmap = (size_t)batch * k * L * 4;
    if (!ranges_disjoint(h, fn, tok8, ntok, "tok8", cam32, nmap, "cam32", OVL_IN) || !ranges_disjoint(h, fn, tok8, ntok, "tok8", map32, nmap, "map32", OVL_IN) ||
        !ranges_disjoint(h, fn, idx, nidx, "idx", cam32, nmap, "cam32", OVL_IN) || !ranges_disjoint(h, fn, idx, nidx, "idx", map32, nmap, "map32", OVL_IN) ||
        !ranges_disjoint(h, fn, cam32, nmap, "cam32", map32, nmap, "map32", OVL_OUT))
        return IVIT_ERR_INVALID;
    if ((C % 16) != 0 || C > CLASSMAP_MAX_C) {
        snprintf(h->err, sizeof(h->err), "%s: C must be a multiple of 16 and at most %d", fn, CLASSMAP_MAX_C);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

extern "C" int ivit_class_map(ivit_handle h, const int8_t *tok8, const int8_t *head_w, const int32_t *idx, int batch, int L, int C, int num_classes,
                              int k, const float *class_scale, int32_t *cam32, float *map32) {
    CHECK_H(h);
    if (const int rc = classmap_args_ok(h, __func__, tok8, head_w, idx, batch, L, C, num_classes, k, class_scale, cam32, map32)) return rc;
    const int BK = batch * k;
    REQUIRE_LAUNCH(h, (BK + 3ll) / 4, 256, 4);
    const unsigned grid = (unsigned)((BK + 3ll) / 4);            // one wavefront per (image, class slot)
    if (map32) class_map_kernel<true><<<grid, 256, 0, h->stream>>>(tok8, head_w, idx, class_scale, cam32, map32, BK, k, L, C, num_classes);
    else class_map_kernel<false><<<grid, 256, 0, h->stream>>>(tok8, head_w, idx, nullptr, cam32, nullptr, BK, k, L, C, num_classes);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- hidden states: the fp32 form of a block's output (include/ivit_hidden.h)
// the argument rules of ivit_hidden_f32 (ivit_model.h asks here for its model's planes, before its slices are launched): pointers, counts,
// the row range, the scale, the layout, alignment, the overlapping pair, then the width
static int hidden_args_ok(ivit_handle h, const char *fn, const int16_t *x16, const char *x_name, float scale, long long batch, int T, int C, int t0,
                          int layout, const float *out, const char *out_name) {
    char bad[96] = "";
    if (!x16 || !out) snprintf(bad, sizeof(bad), "%s or %s is null", x_name, out_name);
    else if (batch < 1 || T < 1 || C < 1) snprintf(bad, sizeof(bad), "batch, T or C is not positive");
    else if (t0 < 0 || t0 >= T) snprintf(bad, sizeof(bad), "t0 must be in [0, T)");
    else if (!(scale > 0.f && scale <= FLT_MAX)) snprintf(bad, sizeof(bad), "scale must be finite and positive");
    else if (layout != IVIT_HIDDEN_TOKENS && layout != IVIT_HIDDEN_GRID) snprintf(bad, sizeof(bad), "layout must be IVIT_HIDDEN_TOKENS or IVIT_HIDDEN_GRID");
    else if ((uintptr_t)x16 & 15) snprintf(bad, sizeof(bad), "%s must be 16-byte aligned", x_name);
    else if ((uintptr_t)out & 15) snprintf(bad, sizeof(bad), "%s must be 16-byte aligned", out_name);
    else if (batch > 0x7fffffffLL || (long long)(T - t0) * C > 0x7fffffffLL * 8) snprintf(bad, sizeof(bad), "batch or an image's rows do not fit an int");
    if (bad[0]) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    if (!ranges_disjoint(h, fn, x16, (size_t)batch * T * C * 2, x_name, out, (size_t)batch * (T - t0) * C * 4, out_name, OVL_IN)) return IVIT_ERR_INVALID;
    if ((C % 8) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: C must be a multiple of 8", fn);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

extern "C" int ivit_hidden_f32(ivit_handle h, const int16_t *x16, float scale, int batch, int T, int C, int t0, int layout, float *out) {
    CHECK_H(h);
    if (const int rc = hidden_args_ok(h, __func__, x16, "x16", scale, batch, T, C, t0, layout, out, "out")) return rc;
    const int N = T - t0;
    const unsigned gy = (unsigned)std::min(batch, 65535);                  // the kernels stride over the images beyond
    if (layout == IVIT_HIDDEN_GRID) {
        const long long tiles = ((N + HIDDEN_TILE - 1ll) / HIDDEN_TILE) * ((C + HIDDEN_TILE - 1ll) / HIDDEN_TILE);
        REQUIRE(h, tiles <= 0x7fffffffLL, "too many tiles for one launch");
        hidden_f32_kernel<true><<<dim3((unsigned)tiles, gy), 256, 0, h->stream>>>(x16, scale, batch, T, C, t0, out);
    } else {
        const long long per = (long long)N * (C / 8);                       // 16-byte pieces of an image: one per thread, strided beyond 2^28
        const unsigned gx = (unsigned)std::min<long long>((per + 255) / 256, 1 << 20);
        hidden_f32_kernel<false><<<dim3(gx, gy), 256, 0, h->stream>>>(x16, scale, batch, T, C, t0, out);
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- gallery search (include/ivit_search.h)
extern "C" int ivit_gallery_inv_norms(ivit_handle h, const int8_t *gallery, int64_t rows, int dim, float *inv_norm) {
    CHECK_H(h);
    REQUIRE(h, gallery && inv_norm && rows >= 0, "gallery or inv_norm is null, or rows is negative");
    REQUIRE_A16(h, gallery, "gallery");
    if (dim < 16 || dim > 65536 || (dim % 16) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 16 in 16 .. 65536", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE_DISJOINT(h, gallery, (size_t)rows * dim, "gallery", inv_norm, (size_t)rows * 4, "inv_norm", OVL_IN);
    if (rows == 0) return IVIT_OK;
    const unsigned grid = (unsigned)std::min<long long>((rows + 15) / 16, 1 << 20);          // 16 rows per block, strided beyond
    gallery_inv_norms_kernel<<<grid, 256, 0, h->stream>>>(gallery, (long long)rows, dim, inv_norm);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// the limits ivit_search_workspace_bytes and ivit_search_topk share, and the number of parts: the caller's, or about two workgroups
// per CU of the handle's share in parts of at least 1024 rows (a part begins with every score surviving and ends with a compaction)
static int search_shape_ok(ivit_handle h, const char *fn, int nq, long long rows, int dim, int k, int splits, int *parts) {
    const char *bad = nullptr;
    if (nq < 0 || rows < 0) bad = "nq or rows is negative";
    else if (k < 1 || k > SEARCH_MAX_K || k > rows) bad = "k must be in 1 .. min(64, rows)";
    else if (splits < 0 || splits > 65535) bad = "splits must be in 0 .. 65535";
    if (bad) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    if (dim < SEARCH_MIN_DIM || dim > SEARCH_MAX_DIM || (dim % 64) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 64 in 64 .. 1024", fn);
        return IVIT_ERR_UNSUPPORTED;
    }
    long long s = splits;
    if (s == 0) {
        const long long cols = std::max(1ll, ((long long)nq + SEARCH_QB - 1) / SEARCH_QB);
        s = std::max(1ll, std::min((2ll * persistent_cus(h) + cols - 1) / cols, rows / 1024));
    }
    *parts = (int)s;
    return IVIT_OK;
}

extern "C" int ivit_search_workspace_bytes(ivit_handle h, int nq, int64_t rows, int dim, int k, int splits, size_t *bytes) {
    CHECK_H(h);
    REQUIRE(h, bytes, "bytes is null");
    int parts = 0;
    if (const int rc = search_shape_ok(h, __func__, nq, rows, dim, k, splits, &parts)) return rc;
    *bytes = (size_t)nq * parts * k * 8;
    return IVIT_OK;
}

// the second phase: the keys of a query in registers where they fit (16 or 64 per lane), rescanned from memory beyond
template <bool PAIRS>
static void search_select_launch(ivit_handle h, const unsigned long long *keys, const int32_t *idx_in, const float *val_in, int nq, long long n, int k,
                                 int32_t *idx, float *val) {
    const unsigned grid = (unsigned)((nq + 3ll) / 4);                       // one wavefront per query
    if (n <= 1024) search_select_kernel<PAIRS, 16><<<grid, 256, 0, h->stream>>>(keys, idx_in, val_in, nq, n, k, idx, val);
    else if (n <= 4096) search_select_kernel<PAIRS, 64><<<grid, 256, 0, h->stream>>>(keys, idx_in, val_in, nq, n, k, idx, val);
    else search_select_kernel<PAIRS, 0><<<grid, 256, 0, h->stream>>>(keys, idx_in, val_in, nq, n, k, idx, val);
}

template <int KS>
static int search_scan_launch(ivit_handle h, dim3 grid, size_t lds, const SearchArgs &a) {
    return launch_dyn<search_scan_kernel<KS, (KS <= SEARCH_PF_MAX_KS)>>(h, grid, dim3(256), lds, a);
}

extern "C" int ivit_search_topk(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight,
                                int k, int32_t index_base, int splits, void *workspace, size_t bytes, int32_t *idx, float *val) {
    CHECK_H(h);
    REQUIRE(h, query && gallery && idx && workspace, "query, gallery, idx or workspace is null");
    int parts = 0;
    if (const int rc = search_shape_ok(h, __func__, nq, rows, dim, k, splits, &parts)) return rc;
    REQUIRE(h, index_base >= 0 && (long long)index_base + rows <= 0x7fffffffLL, "index_base must be >= 0 and index_base + rows <= 2^31 - 1");
    const size_t nws = (size_t)nq * parts * k * 8;
    REQUIRE(h, bytes >= nws, "workspace too small (ivit_search_workspace_bytes)");
    REQUIRE_A16(h, query, "query");
    REQUIRE_A16(h, gallery, "gallery");
    REQUIRE_ALIGNED(h, workspace, "workspace", 8);
    {
        const size_t nout = (size_t)nq * k * 4;
        const struct { const void *p; size_t n; const char *name; } ins[3] = {{query, (size_t)nq * dim, "query"}, {gallery, (size_t)rows * dim, "gallery"},
                                                                           {weight, (size_t)rows * 4, "weight"}};
        for (const auto &i : ins) {
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, idx, nout, "idx", OVL_IN);
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, val, nout, "val", OVL_IN);
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, workspace, bytes, "workspace", OVL_IN);
        }
        REQUIRE_DISJOINT(h, idx, nout, "idx", val, nout, "val", OVL_OUT);
        REQUIRE_DISJOINT(h, idx, nout, "idx", workspace, bytes, "workspace", OVL_OUT);
        REQUIRE_DISJOINT(h, val, nout, "val", workspace, bytes, "workspace", OVL_OUT);
    }
    if (nq == 0) return IVIT_OK;
    SearchArgs a;
    a.query = query; a.gallery = gallery; a.weight = weight; a.ws = (unsigned long long *)workspace;
    a.rows = rows; a.per = (rows + parts - 1) / parts;
    a.nq = nq; a.k = k; a.index_base = index_base; a.parts = parts;
    const dim3 grid((unsigned)(((long long)nq + SEARCH_QB - 1) / SEARCH_QB), (unsigned)parts);
    const size_t lds = search_lds_bytes(k);
    int rc = IVIT_OK;
    switch (dim / 64) {
#define SEARCH_CASE(KS) case KS: rc = search_scan_launch<KS>(h, grid, lds, a); break;
        SEARCH_CASE(1) SEARCH_CASE(2) SEARCH_CASE(3) SEARCH_CASE(4) SEARCH_CASE(5) SEARCH_CASE(6) SEARCH_CASE(7) SEARCH_CASE(8)
        SEARCH_CASE(9) SEARCH_CASE(10) SEARCH_CASE(11) SEARCH_CASE(12) SEARCH_CASE(13) SEARCH_CASE(14) SEARCH_CASE(15) SEARCH_CASE(16)
#undef SEARCH_CASE
    }
    if (rc != IVIT_OK) return rc;
    LAUNCH_CHECK(h);
    search_select_launch<false>(h, a.ws, nullptr, nullptr, nq, (long long)parts * k, k, idx, val);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" int ivit_search_merge(ivit_handle h, const int32_t *idx_in, const float *val_in, int nq, int ncand, int k, int32_t *idx, float *val) {
    CHECK_H(h);
    REQUIRE(h, idx_in && val_in && idx && nq >= 0, "idx_in, val_in or idx is null, or nq is negative");
    REQUIRE(h, k >= 1 && k <= SEARCH_MAX_K && ncand >= k, "k must be in 1 .. min(64, ncand)");
    {
        const size_t nin = (size_t)nq * ncand * 4, nout = (size_t)nq * k * 4;
        REQUIRE_DISJOINT(h, idx_in, nin, "idx_in", idx, nout, "idx", OVL_IN);
        REQUIRE_DISJOINT(h, idx_in, nin, "idx_in", val, nout, "val", OVL_IN);
        REQUIRE_DISJOINT(h, val_in, nin, "val_in", idx, nout, "idx", OVL_IN);
        REQUIRE_DISJOINT(h, val_in, nin, "val_in", val, nout, "val", OVL_IN);
        REQUIRE_DISJOINT(h, idx, nout, "idx", val, nout, "val", OVL_OUT);
    }
    if (nq == 0) return IVIT_OK;
    search_select_launch<true>(h, nullptr, idx_in, val_in, nq, (long long)ncand, k, idx, val);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- linear probe (include/ivit_probe.h)
extern "C" int ivit_probe_accumulate(ivit_handle h, const int8_t *feat8, const int64_t *labels, int64_t rows, int dim, int num_classes, int splits,
                                     int64_t *gram, int64_t *class_sum, int64_t *count) {
    CHECK_H(h);
    REQUIRE(h, feat8 && labels && gram && class_sum && count, "feat8, labels, gram, class_sum or count is null");
    REQUIRE(h, rows >= 0, "rows is negative");
    REQUIRE(h, num_classes >= 1 && num_classes <= PROBE_MAX_CLASSES, "num_classes must be in 1 .. 65536");
    REQUIRE(h, splits >= 0 && splits <= 65535, "splits must be in 0 .. 65535");
    if (dim < PROBE_MIN_DIM || dim > PROBE_MAX_DIM || (dim % 64) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 64 in 64 .. 1024", __func__);
        return IVIT_ERR_UNSUPPORTED;
    }
    REQUIRE_A16(h, feat8, "feat8");
    REQUIRE_ALIGNED(h, labels, "labels", 8);
    REQUIRE_ALIGNED(h, gram, "gram", 8);
    REQUIRE_ALIGNED(h, class_sum, "class_sum", 8);
    REQUIRE_ALIGNED(h, count, "count", 8);
    {
        const struct { const void *p; size_t n; const char *name; } ins[2] = {{feat8, (size_t)rows * dim, "feat8"}, {labels, (size_t)rows * 8, "labels"}},
            outs[3] = {{gram, (size_t)dim * dim * 8, "gram"}, {class_sum, (size_t)num_classes * dim * 8, "class_sum"}, {count, (size_t)num_classes * 8, "count"}};
        for (const auto &i : ins)
            for (const auto &o : outs) REQUIRE_DISJOINT(h, i.p, i.n, i.name, o.p, o.n, o.name, OVL_IN);
        REQUIRE_DISJOINT(h, gram, outs[0].n, "gram", class_sum, outs[1].n, "class_sum", OVL_OUT);
        REQUIRE_DISJOINT(h, gram, outs[0].n, "gram", count, outs[2].n, "count", OVL_OUT);
        REQUIRE_DISJOINT(h, class_sum, outs[1].n, "class_sum", count, outs[2].n, "count", OVL_OUT);
    }
    if (rows == 0) return IVIT_OK;
    ProbeArgs a;
    a.feat8 = feat8; a.labels = (const long long *)labels;
    a.gram = (unsigned long long *)gram; a.class_sum = (unsigned long long *)class_sum; a.count = (unsigned long long *)count;
    a.rows = rows; a.dim = dim; a.num_classes = num_classes; a.nblk = (dim + PROBE_BLK - 1) / PROBE_BLK;
    const long long cus = persistent_cus(h), nrows = rows;
    // the parts of a launch: the caller's count, or the library's; `per` rows each, rounded up to `unit`
    auto parts_of = [&](long long chosen, long long unit, long long *per) {
        const long long s = splits > 0 ? splits : std::max(1ll, std::min(chosen, 65535ll));
        *per = ((nrows + s - 1) / s + unit - 1) / unit * unit;
        return (unsigned)(splits > 0 ? s : (nrows + *per - 1) / *per);
    };
    {   // the Gram matrix: about two workgroups per CU, in parts of at least 4096 rows (a part ends with dim^2 atomic adds per block row)
        const long long pairs = (long long)a.nblk * (a.nblk + 1) / 2;
        const unsigned parts = parts_of(std::min((2 * cus + pairs - 1) / pairs, nrows / 4096), PROBE_CHUNK, &a.per);
        probe_gram_kernel<<<dim3((unsigned)pairs, parts), 256, 0, h->stream>>>(a);
        LAUNCH_CHECK(h);
    }
    {   // class sums and counts: privatised in LDS where [num_classes, dim + 1] int32 fit 64 KB, straight global adds otherwise
        const size_t lds = (size_t)num_classes * (dim + 1) * 4;
        if (lds <= PROBE_CLASS_LDS_BYTES) {
            const unsigned parts = parts_of(std::min(2 * cus, nrows / 256), 1, &a.per);
            probe_class_kernel<true><<<parts, 256, lds, h->stream>>>(a);
        } else {
            const unsigned parts = parts_of((nrows * (dim / 16) + 255) / 256, 1, &a.per);                // about one (row, 16 features) per thread
            probe_class_kernel<false><<<parts, 256, 0, h->stream>>>(a);
        }
        LAUNCH_CHECK(h);
    }
    return IVIT_OK;
}

// ---------------------------------------------------------------- k-means (include/ivit_cluster.h)
// the limits the four entries share
static int kmeans_shape_ok(ivit_handle h, const char *fn, int K, int dim) {
    if (K < 1 || K > KMEANS_MAX_K) {
        snprintf(h->err, sizeof(h->err), "%s: K must be in 1 .. 16384", fn);
        return IVIT_ERR_INVALID;
    }
    if (dim < KMEANS_MIN_DIM || dim > KMEANS_MAX_DIM || (dim % 64) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 64 in 64 .. 1024", fn);
        return IVIT_ERR_UNSUPPORTED;
    }
    return IVIT_OK;
}

extern "C" int ivit_kmeans_norms(ivit_handle h, const int8_t *cent, int K, int dim, int32_t *cnorm) {
    CHECK_H(h);
    REQUIRE(h, cent && cnorm, "cent or cnorm is null");
    if (const int rc = kmeans_shape_ok(h, __func__, K, dim)) return rc;
    REQUIRE_A16(h, cent, "cent");
    REQUIRE_ALIGNED(h, cnorm, "cnorm", 4);
    REQUIRE_DISJOINT(h, cent, (size_t)K * dim, "cent", cnorm, (size_t)K * 4, "cnorm", OVL_IN);
    kmeans_norms_kernel<<<(unsigned)((K + 15) / 16), 256, 0, h->stream>>>(cent, K, dim, cnorm);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

template <int KS>
static void kmeans_assign_launch(ivit_handle h, unsigned grid, const KMeansAssignArgs &a) {
    kmeans_assign_kernel<KS, (KS <= KMEANS_PF_MAX_KS)><<<grid, 256, 0, h->stream>>>(a);
}

extern "C" int ivit_kmeans_assign(ivit_handle h, const int8_t *x, int64_t rows, int dim, const int8_t *cent, const int32_t *cnorm, int K,
                                  int32_t *assign, int32_t *dist2) {
    CHECK_H(h);
    REQUIRE(h, x && cent && cnorm && assign, "x, cent, cnorm or assign is null");
    REQUIRE(h, rows >= 0, "rows is negative");
    if (const int rc = kmeans_shape_ok(h, __func__, K, dim)) return rc;
    REQUIRE_A16(h, x, "x");
    REQUIRE_A16(h, cent, "cent");
    REQUIRE_ALIGNED(h, cnorm, "cnorm", 4);
    REQUIRE_ALIGNED(h, assign, "assign", 4);
    REQUIRE_ALIGNED(h, dist2, "dist2", 4);
    const long long blocks = ((long long)rows + KMEANS_RB - 1) / KMEANS_RB;
    REQUIRE_LAUNCH(h, blocks, 256, KMEANS_RB);
    {
        const size_t nout = (size_t)rows * 4;
        const struct { const void *p; size_t n; const char *name; } ins[3] = {{x, (size_t)rows * dim, "x"}, {cent, (size_t)K * dim, "cent"},
                                                                           {cnorm, (size_t)K * 4, "cnorm"}};
        for (const auto &i : ins) {
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, assign, nout, "assign", OVL_IN);
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, dist2, nout, "dist2", OVL_IN);
        }
        REQUIRE_DISJOINT(h, assign, nout, "assign", dist2, nout, "dist2", OVL_OUT);
    }
    if (rows == 0) return IVIT_OK;
    KMeansAssignArgs a;
    a.x = x; a.cent = cent; a.cnorm = cnorm; a.assign = assign; a.dist2 = dist2; a.rows = rows; a.K = K;
    switch (dim / 64) {
#define KMEANS_CASE(KS) case KS: kmeans_assign_launch<KS>(h, (unsigned)blocks, a); break;
        KMEANS_CASE(1) KMEANS_CASE(2) KMEANS_CASE(3) KMEANS_CASE(4) KMEANS_CASE(5) KMEANS_CASE(6) KMEANS_CASE(7) KMEANS_CASE(8)
        KMEANS_CASE(9) KMEANS_CASE(10) KMEANS_CASE(11) KMEANS_CASE(12) KMEANS_CASE(13) KMEANS_CASE(14) KMEANS_CASE(15) KMEANS_CASE(16)
#undef KMEANS_CASE
    }
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" int ivit_kmeans_accumulate(ivit_handle h, const int8_t *x, const int32_t *assign, const int32_t *dist2, int64_t rows, int dim, int K,
                                      int splits, int64_t *sum, int64_t *count, int64_t *inertia) {
    CHECK_H(h);
    REQUIRE(h, x && assign && sum && count, "x, assign, sum or count is null");
    REQUIRE(h, inertia || !dist2, "inertia is null beside a dist2");
    REQUIRE(h, rows >= 0, "rows is negative");
    REQUIRE(h, splits >= 0 && splits <= 65535, "splits must be in 0 .. 65535");
    if (const int rc = kmeans_shape_ok(h, __func__, K, dim)) return rc;
    REQUIRE_A16(h, x, "x");
    REQUIRE_ALIGNED(h, assign, "assign", 4);
    REQUIRE_ALIGNED(h, dist2, "dist2", 4);
    REQUIRE_ALIGNED(h, sum, "sum", 8);
    REQUIRE_ALIGNED(h, count, "count", 8);
    REQUIRE_ALIGNED(h, inertia, "inertia", 8);
    {
        const struct { const void *p; size_t n; const char *name; } ins[3] = {{x, (size_t)rows * dim, "x"}, {assign, (size_t)rows * 4, "assign"},
                                                                           {dist2, (size_t)rows * 4, "dist2"}},
            outs[3] = {{sum, (size_t)K * dim * 8, "sum"}, {count, (size_t)K * 8, "count"}, {inertia, 8, "inertia"}};
        for (const auto &i : ins)
            for (const auto &o : outs) REQUIRE_DISJOINT(h, i.p, i.n, i.name, o.p, o.n, o.name, OVL_IN);
        REQUIRE_DISJOINT(h, sum, outs[0].n, "sum", count, outs[1].n, "count", OVL_OUT);
        REQUIRE_DISJOINT(h, sum, outs[0].n, "sum", inertia, 8, "inertia", OVL_OUT);
        REQUIRE_DISJOINT(h, count, outs[1].n, "count", inertia, 8, "inertia", OVL_OUT);
    }
    if (rows == 0) return IVIT_OK;
    KMeansAccArgs a;
    a.x = x; a.assign = assign; a.dist2 = dist2;
    a.sum = (unsigned long long *)sum; a.count = (unsigned long long *)count; a.inertia = (unsigned long long *)inertia;
    a.rows = rows; a.dim = dim; a.K = K;
    const long long cus = persistent_cus(h), nrows = rows;
    // the parts: the caller's count, or the library's — privatised in LDS where [K, dim + 1] int32 fit 64 KB, about two workgroups per
    // CU in parts of at least 256 rows (a part ends with a flush of the copy); straight global adds otherwise, 64 rows to a workgroup
    const size_t lds = (size_t)K * (dim + 1) * 4;
    const bool use_lds = lds <= PROBE_CLASS_LDS_BYTES;
    const long long chosen = use_lds ? std::min(2 * cus, nrows / 256) : (nrows + 63) / 64;
    const long long s = splits > 0 ? splits : std::max(1ll, std::min(chosen, 65535ll));
    a.per = (nrows + s - 1) / s;
    const unsigned parts = (unsigned)(splits > 0 ? s : (nrows + a.per - 1) / a.per);
    if (use_lds) kmeans_accumulate_kernel<true><<<parts, 256, lds, h->stream>>>(a);
    else kmeans_accumulate_kernel<false><<<parts, 256, 0, h->stream>>>(a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" int ivit_kmeans_update(ivit_handle h, const int64_t *sum, const int64_t *count, int K, int dim, int8_t *cent, int32_t *cnorm,
                                  int64_t *moved) {
    CHECK_H(h);
    REQUIRE(h, sum && count && cent && cnorm && moved, "sum, count, cent, cnorm or moved is null");
    if (const int rc = kmeans_shape_ok(h, __func__, K, dim)) return rc;
    REQUIRE_A16(h, cent, "cent");
    REQUIRE_ALIGNED(h, cnorm, "cnorm", 4);
    REQUIRE_ALIGNED(h, sum, "sum", 8);
    REQUIRE_ALIGNED(h, count, "count", 8);
    REQUIRE_ALIGNED(h, moved, "moved", 8);
    {
        const struct { const void *p; size_t n; const char *name; } ins[2] = {{sum, (size_t)K * dim * 8, "sum"}, {count, (size_t)K * 8, "count"}},
            outs[3] = {{cent, (size_t)K * dim, "cent"}, {cnorm, (size_t)K * 4, "cnorm"}, {moved, 8, "moved"}};
        for (const auto &i : ins)
            for (const auto &o : outs) REQUIRE_DISJOINT(h, i.p, i.n, i.name, o.p, o.n, o.name, OVL_IN);
        REQUIRE_DISJOINT(h, cent, outs[0].n, "cent", cnorm, outs[1].n, "cnorm", OVL_OUT);
        REQUIRE_DISJOINT(h, cent, outs[0].n, "cent", moved, 8, "moved", OVL_OUT);
        REQUIRE_DISJOINT(h, cnorm, outs[1].n, "cnorm", moved, 8, "moved", OVL_OUT);
    }
    kmeans_update_kernel<<<(unsigned)((K + 3) / 4), 256, 0, h->stream>>>((const long long *)sum, (const long long *)count, K, dim, cent, cnorm,
                                                                         (unsigned long long *)moved);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---------------------------------------------------------------- range search (include/ivit_range.h)
// the workspace: the nq * parts int32 counts, their int64 offsets (8-byte aligned behind the counts) and the scan's block sums
struct RangeLayout {
    long long n, nb;            // counts; blocks of RANGE_SCAN_BLOCK counts
    size_t off, bsum, bytes;    // byte offsets of the offsets and the block sums; the whole
};
static RangeLayout range_layout(int nq, int parts) {
    RangeLayout l;
    l.n = (long long)nq * parts;
    l.nb = (l.n + RANGE_SCAN_BLOCK - 1) / RANGE_SCAN_BLOCK;
    l.off = ((size_t)l.n * 4 + 7) & ~(size_t)7;
    l.bsum = l.off + (size_t)l.n * 8;
    l.bytes = l.bsum + (size_t)l.nb * 8;
    return l;
}

// the limits the three entries share, and the number of parts: the caller's, or that of the search (about two workgroups per CU of the
// handle's share, in parts of at least 1024 rows)
static int range_shape_ok(ivit_handle h, const char *fn, int nq, long long rows, int dim, int splits, int *parts) {
    const char *bad = nullptr;
    if (nq < 0) bad = "nq is negative";
    else if (rows < 1) bad = "rows must be at least 1";
    else if (splits < 0 || splits > 65535) bad = "splits must be in 0 .. 65535";
    if (bad) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    if (dim < SEARCH_MIN_DIM || dim > SEARCH_MAX_DIM || (dim % 64) != 0) {
        snprintf(h->err, sizeof(h->err), "%s: dim must be a multiple of 64 in 64 .. 1024", fn);
        return IVIT_ERR_UNSUPPORTED;
    }
    long long s = splits;
    if (s == 0) {
        const long long cols = std::max(1ll, ((long long)nq + SEARCH_QB - 1) / SEARCH_QB);
        s = std::max(1ll, std::min((2ll * persistent_cus(h) + cols - 1) / cols, rows / 1024));
    }
    if ((long long)nq * s > 0x7fffffffLL) {
        snprintf(h->err, sizeof(h->err), "%s: nq * parts must be at most 2^31 - 1", fn);
        return IVIT_ERR_INVALID;
    }
    *parts = (int)s;
    return IVIT_OK;
}

extern "C" int ivit_range_workspace_bytes(ivit_handle h, int nq, int64_t rows, int dim, int splits, size_t *bytes) {
    CHECK_H(h);
    REQUIRE(h, bytes, "bytes is null");
    int parts = 0;
    if (const int rc = range_shape_ok(h, __func__, nq, rows, dim, splits, &parts)) return rc;
    *bytes = range_layout(nq, parts).bytes;
    return IVIT_OK;
}

// what ivit_range_count and ivit_range_fill check alike, in the same order, and the kernel's arguments
static int range_args_ok(ivit_handle h, const char *fn, const int8_t *query, int nq, const int8_t *gallery, long long rows, int dim, const float *weight,
                         const float *qweight, float threshold, int index_base, int query_base, int triangle, int splits, void *workspace, size_t bytes,
                         RangeArgs *a, RangeLayout *l) {
    int parts = 0;
    if (const int rc = range_shape_ok(h, fn, nq, rows, dim, splits, &parts)) return rc;
    const char *bad = nullptr;
    if (index_base < 0 || (long long)index_base + rows > 0x7fffffffLL) bad = "index_base must be >= 0 and index_base + rows <= 2^31 - 1";
    else if (query_base < 0 || (long long)query_base + nq > 0x7fffffffLL) bad = "query_base must be >= 0 and query_base + nq <= 2^31 - 1";
    else if (!(threshold >= -FLT_MAX && threshold <= FLT_MAX)) bad = "threshold must be finite";
    *l = range_layout(nq, parts);
    if (!bad && bytes < l->bytes) bad = "workspace too small (ivit_range_workspace_bytes)";
    if (!bad && ((uintptr_t)query & 15)) bad = "query must be 16-byte aligned";
    if (!bad && ((uintptr_t)gallery & 15)) bad = "gallery must be 16-byte aligned";
    if (!bad && ((uintptr_t)workspace & 7)) bad = "workspace must be 8-byte aligned";
    if (bad) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, bad); return IVIT_ERR_INVALID; }
    a->query = query; a->gallery = gallery; a->weight = weight; a->qweight = qweight;
    a->cnt = (int *)workspace; a->off = (const long long *)((char *)workspace + l->off);
    a->idx = nullptr; a->val = nullptr;
    a->rows = rows; a->per = (rows + parts - 1) / parts; a->capacity = 0;
    a->threshold = threshold;
    a->nq = nq; a->index_base = index_base; a->query_base = query_base; a->triangle = triangle != 0; a->parts = parts;
    return IVIT_OK;
}

template <int KS, bool FILL>
static void range_scan_launch(ivit_handle h, dim3 grid, const RangeArgs &a) {
    range_scan_kernel<KS, (KS <= SEARCH_PF_MAX_KS), FILL><<<grid, 256, 0, h->stream>>>(a);
}

template <bool FILL>
static void range_scan_dispatch(ivit_handle h, int dim, const RangeArgs &a) {
    const dim3 grid((unsigned)(((long long)a.nq + SEARCH_QB - 1) / SEARCH_QB), (unsigned)a.parts);
    switch (dim / 64) {
#define RANGE_CASE(KS) case KS: range_scan_launch<KS, FILL>(h, grid, a); break;
        RANGE_CASE(1) RANGE_CASE(2) RANGE_CASE(3) RANGE_CASE(4) RANGE_CASE(5) RANGE_CASE(6) RANGE_CASE(7) RANGE_CASE(8)
        RANGE_CASE(9) RANGE_CASE(10) RANGE_CASE(11) RANGE_CASE(12) RANGE_CASE(13) RANGE_CASE(14) RANGE_CASE(15) RANGE_CASE(16)
#undef RANGE_CASE
    }
}

extern "C" int ivit_range_count(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight,
                                const float *qweight, float threshold, int32_t index_base, int32_t query_base, int triangle, int splits,
                                void *workspace, size_t bytes, int64_t *row_ptr) {
    CHECK_H(h);
    REQUIRE(h, query && gallery && workspace && row_ptr, "query, gallery, workspace or row_ptr is null");
    RangeArgs a;
    RangeLayout l;
    if (const int rc = range_args_ok(h, __func__, query, nq, gallery, rows, dim, weight, qweight, threshold, index_base, query_base, triangle, splits,
                                     workspace, bytes, &a, &l)) return rc;
    REQUIRE_ALIGNED(h, row_ptr, "row_ptr", 8);
    {
        const size_t nrp = ((size_t)nq + 1) * 8;
        const struct { const void *p; size_t n; const char *name; } ins[4] = {{query, (size_t)nq * dim, "query"}, {gallery, (size_t)rows * dim, "gallery"},
                                                                           {weight, (size_t)rows * 4, "weight"}, {qweight, (size_t)nq * 4, "qweight"}};
        for (const auto &i : ins) {
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, workspace, bytes, "workspace", OVL_IN);
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, row_ptr, nrp, "row_ptr", OVL_IN);
        }
        REQUIRE_DISJOINT(h, workspace, bytes, "workspace", row_ptr, nrp, "row_ptr", OVL_OUT);
    }
    if (nq == 0) return IVIT_OK;
    range_scan_dispatch<false>(h, dim, a);
    LAUNCH_CHECK(h);
    long long *off = (long long *)((char *)workspace + l.off), *bsum = (long long *)((char *)workspace + l.bsum);
    range_block_sums_kernel<<<(unsigned)l.nb, 256, 0, h->stream>>>(a.cnt, l.n, bsum);
    LAUNCH_CHECK(h);
    range_scan_sums_kernel<<<1, 256, 0, h->stream>>>(bsum, l.nb, (long long *)row_ptr + nq);
    LAUNCH_CHECK(h);
    range_offsets_kernel<<<(unsigned)l.nb, 256, 0, h->stream>>>(a.cnt, bsum, l.n, a.parts, off, (long long *)row_ptr);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

extern "C" int ivit_range_fill(ivit_handle h, const int8_t *query, int nq, const int8_t *gallery, int64_t rows, int dim, const float *weight,
                               const float *qweight, float threshold, int32_t index_base, int32_t query_base, int triangle, int splits,
                               void *workspace, size_t bytes, int64_t capacity, int32_t *idx, float *val) {
    CHECK_H(h);
    REQUIRE(h, query && gallery && workspace && idx, "query, gallery, workspace or idx is null");
    REQUIRE(h, capacity >= 0, "capacity is negative");
    RangeArgs a;
    RangeLayout l;
    if (const int rc = range_args_ok(h, __func__, query, nq, gallery, rows, dim, weight, qweight, threshold, index_base, query_base, triangle, splits,
                                     workspace, bytes, &a, &l)) return rc;
    {
        const size_t nout = (size_t)capacity * 4;
        const struct { const void *p; size_t n; const char *name; } ins[5] = {{query, (size_t)nq * dim, "query"}, {gallery, (size_t)rows * dim, "gallery"},
                                                                           {weight, (size_t)rows * 4, "weight"}, {qweight, (size_t)nq * 4, "qweight"},
                                                                           {workspace, bytes, "workspace"}};
        for (const auto &i : ins) {
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, idx, nout, "idx", OVL_IN);
            REQUIRE_DISJOINT(h, i.p, i.n, i.name, val, nout, "val", OVL_IN);
        }
        REQUIRE_DISJOINT(h, idx, nout, "idx", val, nout, "val", OVL_OUT);
    }
    if (nq == 0 || capacity == 0) return IVIT_OK;
    a.idx = idx; a.val = val; a.capacity = capacity;
    range_scan_dispatch<true>(h, dim, a);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

#include "ivit_model.h"
#include "ivit_modelfile.h"      // behind the runners: ivit_model_open ends in ivit_vit_create / ivit_swin_create
