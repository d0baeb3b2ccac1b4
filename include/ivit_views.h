/*
 * ivit_views.h — image views: a box of an image, resized as PIL resizes a stand-alone image, a crop x crop window of that, optionally
 * mirrored; any number of views of any images of a ragged batch in ONE launch.  Regions (a detector's boxes, tiles of a scan),
 * five-crop / ten-crop evaluation and augmented views for a probe are all this one operation.  And the exact combination of the
 * views' outputs: the integer sum of the int32 logits of the views of one image.  Tenth public header of libivit_hip.so.
 *
 * Why a tenth header: ivit.h is frozen at IVIT_VERSION 111 and the eight headers behind it at their versions 1 (their prototypes
 * and versions are pinned by the binding's tests), so these entries are declared here, under a version of their own.  This header
 * includes ivit.h and uses its handle (ivit_handle), its image descriptor (ivit_image_desc), its status codes and every one of its
 * conventions: device pointers unless a name ends in _host, dense row-major tensors, asynchronous on the handle's HIP stream, nothing
 * allocated, nothing synchronised, hipGraph-capturable, IVIT_OK or an error code; a pointer named in an "Alignment:" line is refused
 * with IVIT_ERR_INVALID unless aligned, and a pair named in an "Overlap:" line unless disjoint (ivit_last_error then contains
 * "overlap" and both names), before anything is launched.
 *
 * The definition (ivit_amd/views.py: views_reference is the numpy statement, tests/golden/pil_views.npz — written by Pillow — the pin):
 *   view = Image.crop((x0, y0, x0 + bw, y0 + bh)).resize((rw, rh), Image.BICUBIC).crop((left, top, left + crop, top + crop))
 *   then .transpose(Image.FLIP_LEFT_RIGHT) where flip is 1.
 * PIL resamples the box as a stand-alone image: the taps clamp at the BOX's edges, so a view depends on no byte outside its box.  It
 * is the arithmetic of ivit_resize_center_crop_u8_pil (ivit.h; csrc/ivit_preprocess.h states it line by line) on a sub-image whose
 * row stride is the image's: coefficients in double, 22-bit fixed point, horizontal pass into uint8, then vertical; an axis whose
 * length does not change (rw == bw, rh == bh) is copied.  The eval transform's view of an image is the box of the whole image, (rw,
 * rh) its resized size and (left, top) the centre crop's offsets: ivit_amd.views.center_views.
 *
 * Deliberately not here: the mean of probabilities (the mean LOGIT is what exact integers give); sharing the resize work between the
 * views of one image (each view builds its own taps); vertical flips, rotations, colour jitter; float boxes (resize(box=...));
 * a runner-level entry or graph form (the three entries are capturable: a caller's graph can hold them).
 */
#ifndef IVIT_VIEWS_H
#define IVIT_VIEWS_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_view_resize_u8_pil, ivit_view_transform_u8, ivit_logits_view_sum. */
#define IVIT_VIEWS_VERSION 1

/* One view: see the definition above. */
typedef struct ivit_view_desc {
    int32_t image;             /* index into the image table (ivit_image_desc [B]) */
    int32_t x0, y0, bw, bh;    /* source box inside that image */
    int32_t rw, rh;            /* PIL size=(rw, rh) the box is resized to */
    int32_t left, top;         /* crop x crop window of the resized box */
    int32_t flip;              /* 0, or 1: mirrored left-right */
} ivit_view_desc;              /* 40 bytes */

/* ---- v1  V views of the B images of a ragged batch, one launch: out_hwc uint8 [V, crop, crop, 3], PIL's bytes of the definition
 * above (every byte, no tolerance).  pixels / pixels_bytes / img_host / img_dev / B are the ragged batch of
 * ivit_resize_center_crop_u8_pil; view_host and view_dev are the SAME V records, on the host and on the device (the caller places
 * the device copy).  The call validates the host tables before anything is launched — per image what ivit_resize_center_crop_u8_pil
 * checks (h, w > 0; offset >= 0; offset + h * w * 3 <= pixels_bytes), per view 0 <= image < B; bw, bh >= 1 and the box inside the
 * image (x0, y0 >= 0; x0 + bw <= w; y0 + bh <= h); 1 <= rw, rh <= 65536; the window inside the resized box (left, top >= 0; left +
 * crop <= rw; top + crop <= rh); flip 0 or 1 — and on a failed check returns IVIT_ERR_INVALID with the image's or the view's index
 * in ivit_last_error ("view 3: ..."), nothing launched.  The kernel reads ONLY the device tables: a replay of a captured graph reads
 * them again, so whatever they hold then must describe images and views for which the captured call's checks hold.  The host
 * descriptor tables are read at call time by design: a captured call keeps the launch shape it took from them, and a replay may
 * bring other pixel bytes under the same descriptors.  B >= 1, crop >=
 * 1, V >= 0; with V == 0 nothing is launched (view_host and view_dev may then be NULL).  ceil(crop / 32) * V blocks of 512 threads
 * must stay below 2^32 work-items: IVIT_ERR_INVALID otherwise.  No workspace.
 * Alignment: none: pixels, the offsets and out_hwc take any address (byte accesses only), the tables are aligned as their structs.
 * Overlap: out_hwc may not overlap pixels (all pixels_bytes of it), img_dev or view_dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_view_resize_u8_pil(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *img_host,
                            const ivit_image_desc *img_dev, int B, const ivit_view_desc *view_host, const ivit_view_desc *view_dev,
                            int V, int crop, uint8_t *out_hwc);

/* ---- v2  the same views taken through the 3 x 256 table of ivit_normalize_quantize_u8 (ivit.h) with the HWC -> CHW transpose: nchw
 * int8 [V, 3, crop, crop], what the models read; the uint8 crop is never written to memory.  Equal, byte for byte, to
 * ivit_normalize_quantize_u8 on the bytes of ivit_view_resize_u8_pil.  Tables, checks, graph replay as above; mean_host / std_host
 * are HOST arrays of 3 floats, std_host without a zero, scale > 0.
 * Alignment: none: pixels, the offsets and nchw take any address (byte accesses only), the tables are aligned as their structs.
 * Overlap: nchw may not overlap pixels (all pixels_bytes of it), img_dev or view_dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_view_transform_u8(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *img_host,
                           const ivit_image_desc *img_dev, int B, const ivit_view_desc *view_host, const ivit_view_desc *view_dev,
                           int V, int crop, const float mean_host[3], const float std_host[3], float scale, int8_t *nchw);

/* ---- v3  the views of one image share the head's per-class scale, so their MEAN logit is the integer sum of their int32 logits
 * times scale / views.  logits int32 [groups * views, num_classes], the views of a group in consecutive rows -> out int32 [groups,
 * num_classes]:
 *   out[g, c] = clip(sum_{v < views} (int64)logits[g * views + v, c], INT32_MIN, INT32_MAX)
 * accumulated in 64 bits and SATURATED to int32 (ivit_amd.predict.view_sum_reference states it with np.clip).  ivit_logits_topk and
 * ivit_logits_score (ivit.h, ivit_eval.h) of `out` with the scale vector fl32(scale[c] / fl32(views)) give the values, the order
 * and the loss of the mean logits.  1 <= views <= 64, groups >= 0 (0: nothing launched), num_classes >= 1: IVIT_ERR_INVALID
 * otherwise.  One launch, a plain stream.
 * Alignment: none: logits and out take any int32 address (16-byte accesses are used where both are 16-byte aligned and num_classes
 * is a multiple of 4, 4-byte accesses otherwise).
 * Overlap: out may not overlap logits: IVIT_ERR_INVALID, nothing launched. */
int ivit_logits_view_sum(ivit_handle h, const int32_t *logits, int groups, int views, int num_classes, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_VIEWS_H */
