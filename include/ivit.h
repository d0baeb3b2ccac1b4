/*
 * ivit.h — C-ABI of the MI355X-native integer-only ViT inference path.
 *
 * The reference (zkkli/I-ViT) has no FFI layer: its boundary for this path is the
 * Python operator surface of models/quantization_utils/quant_modules.py (re-exported
 * by models/quantization_utils/__init__.py:1).  Each entry point below names the
 * reference interface it replaces (file:line, relative to the reference root).  The
 * Python face that mirrors the reference classes lives in i-vit_amd/quant_modules.py
 * and binds these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - tensors are dense row-major, the channel dimension is last;
 *   - every call is asynchronous on the handle's HIP stream, allocates nothing,
 *     synchronises nothing and is hipGraph-capturable;
 *   - return value: IVIT_OK or an error code (no exceptions, no aborts);
 *   - alignment: an activation or output pointer that a kernel touches through vector accesses wider than its element must be
 *     aligned to that width, 16 bytes unless stated: a misaligned one is refused with IVIT_ERR_INVALID before anything is
 *     launched, and ivit_last_error names the argument.  The "Alignment:" line in front of an entry lists the pointers this
 *     applies to; an activation or output pointer it does not list (and every one of an entry without such a line) takes any
 *     address aligned to its element — a row sub-view with an odd pitch, a slice of a batch.  Weights, biases, dyadic tables,
 *     LayerNorm constants and Shiftmax tables are read in 16-byte pieces throughout: keep them 16-byte aligned (a
 *     256-byte-aligned constants blob does);
 *   - overlapping arguments: an array an entry writes — an output, or a scratch such as scratch8 or a workspace — may overlap
 *     neither an activation array the entry reads nor another array it writes.  Overlap is judged on extents, [p, p + extent) in
 *     bytes, where extent is the span this header documents the entry as addressing: a dense [rows, n] array is rows * n elements,
 *     a pitched or strided one (ld, ldv, lds, ldp, the row_stride of ivit_layernorm_requant and ivit_gather_rows_i16, the batch
 *     strides of ivit_bmm_nt_*) is (rows - 1) * pitch + row payload, pad columns between rows included.  An overlapping call is
 *     refused with IVIT_ERR_INVALID before anything is launched, before any decision that would yield IVIT_ERR_UNSUPPORTED (the
 *     row-table attention entries judge their multipliers' range first, as they always did), and ivit_last_error contains the word
 *     "overlap" and the two argument names.  Arrays that merely touch are accepted.  Two inputs may overlap freely.  Weights,
 *     biases, dyadic tables, LUTs and whatever a plan holds are constants: the caller must not write them during a call, and they are
 *     not checked.  The "Overlap:" line in front of an entry states its rule.  ONE entry declares an (input, output) pair in place,
 *     ivit_linear_i8_requant_residual with residual == out (the reference's x = x + f(x)): the SAME pointer with the SAME extent is
 *     accepted and gives, bit for bit, the bytes of the call on disjoint arrays; every other overlap of that pair is still refused.
 *     The planned and fused forms of the identity branch need a second buffer (ping-pong x / y as ivit_vit_forward does).  The
 *     whole-model runners refuse images, workspace and logits that overlap, and the predict entries idx and val against those three
 *     and each other, before the forward is launched;
 *   - rows per call: a launch holds fewer than 2^32 work-items (blocks x threads; the runtime would take more modulo 2^32 without
 *     an error).  An entry whose grid grows with its row count refuses a call beyond that with IVIT_ERR_UNSUPPORTED before anything
 *     is launched, and ivit_last_error says "2^32 work-items" and the largest row count one call takes: (2^24 - 1) * 4 = 67 108 860
 *     rows for ivit_shiftmax, ivit_shiftmax_masked, ivit_shiftgelu, ivit_shiftgelu_requant, and as many images for ivit_logits_topk
 *     and for the entries of the other headers that work one image (row, head, class slot) per wavefront;
 *     (2^24 - 1) * 8 rows for ivit_layernorm; (2^24 - 1) * 32 for ivit_layernorm_requant at the dispatched widths (C = 96 .. 384;
 *     (2^23 - 1) * 32 at C = 512 .. 1536) and for the token-order LayerNorms; 2^23 - 1 (image, head) pairs for the fused attention
 *     entries.  ivit_shiftgelu_requant_lut, the element-wise entries (requant, quantize, widen) and the GEMMs take any row count
 *     (ranges of 2^25 rows per launch; grid-stride loops);
 *   - activations are carried as INTEGERS plus an fp32 scale held by the caller
 *     (the reference carries fp32 "integer*scale" tensors; X = fl(Q*s) is
 *     re-derived inside the kernels where its rounding matters).
 *
 * Dyadic requantisation (reference quant_utils.py:150-175, 213-253):
 *   out = clamp( rne( (double(z) * m) * r ) [+ rne((double(z_id) * m_id) * r_id)] )
 *   with m = round_half_away(mant * 2^31), r = 2^-(31 - exponent) of
 *   double(s_pre)/double(float(s_out)); prepared on the host (ivit_amd.freeze).
 */
#ifndef IVIT_H
#define IVIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivit_ctx *ivit_handle;

typedef struct ivit_dyadic {
    double m; /* integer-valued multiplier, |m| <= 2^31 (negative after LN with w<0) */
    double r; /* 2^-e */
} ivit_dyadic;

enum {
    IVIT_OK = 0,
    IVIT_ERR_INVALID = 1,     /* bad argument (null pointer, size, alignment, bits) */
    IVIT_ERR_HIP = 2,         /* HIP runtime error, see ivit_last_error            */
    IVIT_ERR_UNSUPPORTED = 3, /* shape outside what the kernels are built for      */
    IVIT_ERR_NO_DEVICE = 4
};

/* 100 * major + minor.  111: ivit_layernorm_mlp_lockstep_planned, ivit_vit_fused_ln_mlp_blocks (additions only): ivit_vit_forward
 * runs norm2 + the Mlp of a D = 192 block, and of a D = 384 block below two units per CU (small batches, the class-token tail), as
 * one launch.
 * 110: ivit_linear_plan_prepare_ws also takes K = 192 plans, and every entry that runs on a prepared plan takes
 * them (ivit_linear_i8_qkv_planned also with v^T there); ivit_layernorm_linear_i8_qkv_ldv_planned, ivit_vit_fused_qkv_blocks
 * (additions only): ivit_vit_forward runs norm1 + qkv of a D = 192, dh = 64 block as one launch and its attn.proj on the same kernel.
 * 109: the class-token forms of the fused attention (ivit_attention_fused_cls, ivit_attention_fused_lut_cls,
 * ivit_attention_fused_rowlut_cls), ivit_gather_rows_i16, ivit_vit_cls_tail (additions only): ivit_vit_forward runs the last
 * block's attention, proj, norm2 and Mlp on the class-token rows only.
 * 108: ivit_mlp_plan_create also takes 256 -> 1024 -> 256 and ivit_mlp_fused also C = 128, hidden = 512
 * (Swin-B stages 1 and 0); no prototype changed, no entry added.
 * 107: ivit_mlp_plan_create also takes 192 -> 768 -> 192 (DeiT-Tiny, Swin stage 1);
 * ivit_vit_fused_mlp_blocks, ivit_swin_fused_mlp_blocks (additions only).
 * 106: the debug entry that copied a plan's store scratch to the host is gone (only probe builds wrote it).
 * 105: ivit_avgpool_requant_scaled (addition); ivit_swin_params gains s_pool at its END — ivit_swin_create
 * copies the whole struct, so a caller compiled against an older header must be rebuilt (its struct is shorter than the
 * library reads); windows 12 in ivit_window_attention_fused / ivit_swin_create.
 * 104 (round 6): ivit_set_cu_share, ivit_linear_i8_requant8_store16 (additions only).
 * 103 (round 6): ivit_linear_plan_prepare_ws, ivit_layernorm_linear_i8_qkv_planned,
 * ivit_linear_i8_requant_residual_layernorm_planned, ivit_layernorm_linear_i8_requant_planned, ivit_patch_embed,
 * ivit_layernorm_mlp_fused_planned (additions only).
 * 102 (round 6): ivit_shiftmax_rowtable, ivit_attention_fused_rowlut (additions only).
 * 101 (round 5): ivit_mlp_plan_select; ivit_swin_block / ivit_vit_block carry the optional Shiftmax-table
 * fields exp_* at their END (added in 100 without a bump: a caller compiled against an older layout must be rebuilt).
 * Parameter structs are read field by field: ZERO-INITIALISE them (memset / = {0}) before filling — exp_aq == NULL (and
 * exp_nc == exp_tcount == exp_dmin == 0) selects the arithmetic Shiftmax, anything else is taken as device pointers.        */
#define IVIT_VERSION 111
int ivit_version(void);
const char *ivit_status_string(int status);

/* One handle per (device, stream).  `hip_stream` is a hipStream_t (NULL = default). */
int ivit_create(ivit_handle *out, int device, void *hip_stream);
int ivit_destroy(ivit_handle h);
int ivit_set_stream(ivit_handle h, void *hip_stream);
/* CUs the one-workgroup-per-CU kernels launched through `h` (the K = 384 QuantLinear layers on gemm_ws_qkv_kernel, the fused Mlp) size their
 * grids for; 0 (the default) = every CU of the device.  A caller that runs several handles side by side on slices of a batch — what
 * ivit_vit_forward / ivit_swin_forward do internally with nslices > 1 — gives each handle its share (CUs / slices): a slice's launch then
 * has the per-workgroup geometry of the unsliced one and the slices' kernels run on disjoint CUs (Swin-T b256, two slices: +2.0 %).
 * The window-12 attention sizes its windows per block for the share too (fewer CUs: more windows per block).
 * No reference counterpart (the reference has no launch geometry); results do not depend on it. */
int ivit_set_cu_share(ivit_handle h, int cus);
const char *ivit_last_error(ivit_handle h);

/* ---- a4  QuantAct.forward, input branch  (quant_modules.py:194-196 ->
 * quant_utils.py:77-96, 12-48):  q = clamp(rne(fl(fl(1/s)*x)), -128, 127)            */
/* Alignment: x 16-byte aligned, q 4-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: q may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_quantize_input_f32(ivit_handle h, const float *x, float scale, int8_t *q, int64_t n);
/* ToTensor -> Normalize(mean, std) -> the same input QuantAct, from uint8 pixels on the device
 * (utils/data_utils.py:89-91: transforms.ToTensor, transforms.Normalize; then vit_quant.py:257):
 * hwc uint8 [B, H, W, 3] (a centre-cropped image as PIL hands it over) -> nchw int8 [B, 3, H, W].
 * mean / std are HOST arrays of 3 floats.  Resize / crop: ivit_resize_center_crop_u8 below.       */
/* Overlap: nchw may not overlap hwc: IVIT_ERR_INVALID, nothing launched. */
int ivit_normalize_quantize_u8(ivit_handle h, const uint8_t *hwc, int B, int H, int W, const float mean_host[3],
                               const float std_host[3], float scale, int8_t *nchw);

/* Resize(size, interpolation=bicubic) + CenterCrop(crop) of the same eval transform (utils/data_utils.py:82-88) on the
 * device: hwc uint8 [B, H0, W0, 3] -> out_hwc uint8 [B, crop, crop, 3] (feed it to ivit_normalize_quantize_u8).  The
 * shorter side is resized to `size` (the longer to int(size * long / short)), antialiased separable bicubic (a = -0.5)
 * in fp32, rne, clamp; then the centre crop.  workspace: B * H0 * crop * 3 floats (caller-owned).
 * Two front ends restate that transform, and they are pinned to different things:
 *   - this entry is pinned to TORCH's antialiased bicubic (tests/golden/resize.npz, within 1 LSB on < 1e-3 of the pixels).  It
 *     is not what the reference computes: the reference resizes PIL images, and PIL's filter differs from torch's by more than
 *     rounding (22-bit fixed point, a uint8 intermediate between the two passes);
 *   - ivit_resize_center_crop_u8_pil and ivit_eval_transform_u8 below are pinned to PIL's own bytes
 *     (tests/golden/pil_resize.npz) and take images of different sizes in one call.  A count that is to equal the
 *     reference's `quant_train.py --evaluate` goes through those.                                                         */
/* Overlap: workspace and out_hwc may overlap neither hwc nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_resize_center_crop_u8(ivit_handle h, const uint8_t *hwc, int B, int H0, int W0, int size, int crop,
                               float *workspace, uint8_t *out_hwc);

/* One image of a ragged batch: h * w * 3 bytes at pixels + offset, uint8 HWC, dense.  No alignment requirement on offset. */
typedef struct ivit_image_desc {
    int64_t offset;
    int32_t h, w;
} ivit_image_desc;

/* Resize(size, interpolation=3) + CenterCrop(crop) of the reference's eval transform (utils/data_utils.py:82-92:
 * transforms.Resize on PIL images, then transforms.CenterCrop) for B images of DIFFERENT sizes, in one launch, bit-exact with
 * PIL: the pin is PIL's own output, Image.resize((Wr, Hr), Image.BICUBIC) then the crop (tests/golden/pil_resize.npz; every byte,
 * no tolerance).  Sizes and crop offsets follow torchvision, as in ivit_resize_center_crop_u8: the shorter side becomes `size`,
 * the longer int(size * long / short) in integers; offsets rint((dim - crop) / 2.0), ties to even.  The arithmetic is PIL's:
 * coefficients in double, 22-bit fixed point, horizontal pass into uint8, then vertical; an axis whose length does not change
 * is copied (csrc/ivit_preprocess.h states it line by line, ivit_amd.preprocess.pil_resize_center_crop_reference in numpy).
 * out_hwc uint8 [B, crop, crop, 3].
 * desc_host and desc_dev are the SAME B records, on the host and on the device (the caller places the device copy, as it places
 * every other constant).  The call validates the host copy — h, w > 0; offset >= 0; offset + h * w * 3 <= pixels_bytes; crop <=
 * both resized sides — and on a failed check returns IVIT_ERR_INVALID with the image's index in ivit_last_error, nothing
 * launched.  The kernel reads ONLY the device copy: a replay of a captured graph reads the device table again, so whatever it
 * holds then must describe images for which the captured call's checks hold (inside pixels_bytes, crop inside the resized image).
 * The host descriptor table is read at call time by design: a captured call keeps the launch shape it took from it, and a replay
 * may bring other pixel bytes under the same descriptors.
 * Every image that ivit_resize_center_crop_u8 accepts is accepted.  No workspace.  pixels, the offsets and the output take any
 * address (byte accesses only).
 * Overlap: out_hwc may not overlap pixels (all pixels_bytes of it) or desc_dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_resize_center_crop_u8_pil(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *desc_host,
                                   const ivit_image_desc *desc_dev, int B, int size, int crop, uint8_t *out_hwc);

/* The whole eval transform of the reference (utils/data_utils.py:82-92: Resize, CenterCrop, ToTensor, Normalize; then the input
 * QuantAct, vit_quant.py:257) on a ragged batch in one launch: the bytes of ivit_resize_center_crop_u8_pil taken through the
 * 3 x 256 table of ivit_normalize_quantize_u8 with the HWC -> CHW transpose, nchw int8 [B, 3, crop, crop]; the cropped uint8
 * image is never written.  Equal, byte for byte, to ivit_normalize_quantize_u8 on PIL's bytes: the pin is PIL
 * (tests/golden/pil_resize.npz).  Descriptors, checks, graph replay and alignment as above; mean_host / std_host are HOST
 * arrays of 3 floats.
 * Overlap: nchw may not overlap pixels (all pixels_bytes of it) or desc_dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_eval_transform_u8(ivit_handle h, const uint8_t *pixels, size_t pixels_bytes, const ivit_image_desc *desc_host,
                           const ivit_image_desc *desc_dev, int B, int size, int crop, const float mean_host[3],
                           const float std_host[3], float scale, int8_t *nchw);

/* ---- a1  QuantLinear.forward  (quant_modules.py:67-97) — integer accumulators.
 * acc[i,j] = sum_k x[i,k]*w[j,k] + bias[j];  x int8 [M,K], w int8 [N,K], K % 16 == 0. */
/* Alignment: x 16-byte aligned; acc takes any int32 address (a slice of a batch's logits); IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: acc may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                   int32_t *acc, int M, int N, int K);

/* a1 + a3: the QuantLinear -> QuantAct pairs of the reference, fused.
 * out = clamp_bits(rq(acc[i,j], dy_ch[j]));  bits = 8 (int8 out) or 16 (int16 out).    */
/* Alignment: x and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                           const ivit_dyadic *dy_ch, int bits, void *out, int M, int N, int K);

/* a1 + a3 + a3(identity): proj/fc2 -> QuantAct(16) -> Block.qact2/qact4 residual add
 * (vit_quant.py:84-85,135,141; layers_quant.py:150-151):
 * t = clamp16(rq(acc, dy_ch[j])); out = clamp16(rq(t, dy_main) + rq(residual, dy_res)). */
/* Alignment: x, residual and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: residual == out (the same pointer, the same extent) is the in place form and gives the bytes of the call on disjoint arrays. Any other overlap of out with x or residual: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant_residual(ivit_handle h, const int8_t *x, const int8_t *w,
                                    const int32_t *bias, const ivit_dyadic *dy_ch,
                                    ivit_dyadic dy_main, ivit_dyadic dy_res,
                                    const int16_t *residual, int16_t *out, int M, int N, int K);

/* a1 + a3 + head split (vit_quant.py:61-69): qkv Linear -> QuantAct(8) -> q,k as
 * [B,H,T,dh] and v TRANSPOSED as [B,H,dh,ldv] (token dim contiguous, ldv % 16 == 0,
 * ldv >= T) — the layout the MFMA attn·v operand wants.  x is [B*T, D], w [3D, D].
 * ldv == 0 (round 6): v ROW-major [B,H,T,dh] like q and k, for ivit_attention_fused_rowlut(ldv = 0).
 * Columns t >= T of v^T are not written (by the _planned form neither), and no entry that takes v^T or a padded uint16 p
 * (ivit_bmm_nt_u16i8, ivit_attn_pv_requant, ivit_attention_fused*) reads them: they need not be zero. */
/* Alignment: x, q, k and vt 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: q, k and vt may overlap neither x nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_qkv(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias,
                       const ivit_dyadic *dy_ch, int8_t *q, int8_t *k, int8_t *vt, int B, int T,
                       int H, int dh, int ldv);

/* ---- constants: one packed byte blob per frozen model (int8 weights, int32 biases, dyadic tables, position
 * embedding; layout = the host packer's table) — how a C host distributes them without
 * Python or torch.distributed (SURVEY.md §8b minimum surface, §8e).  Replaces the reference's per-GPU
 * `model.cuda()` of fp32 parameters + per-forward re-quantisation (quant_modules.py:68-91).
 * upload: host -> device on the handle's stream (asynchronous; the host buffer must stay valid until the stream
 * reaches it).  broadcast: in-place ncclBroadcast of the device blob from rank `root` over a caller-supplied RCCL
 * communicator (ncclComm_t), enqueued on the handle's stream — ONE large message, ring over xGMI; the only
 * collective of the data-parallel path.  librccl.so is resolved at first use.                                   */
int ivit_constants_upload(ivit_handle h, const void *host_blob, size_t bytes, void *device_blob);
int ivit_constants_broadcast(ivit_handle h, void *device_blob, size_t bytes, int root, void *rccl_comm);

/* ---- linear plans: a frozen QuantLinear prepared once (quant_modules.py:67-97 with QuantAct.fix(), :153-157).
 * ivit_linear_plan_create precomputes the per-channel multipliers c[n] = m*2^-e and checks, from
 * sum_k |w[n,k]| and bias[n], the two bounds under which the persistent pipelined GEMM (csrc/ivit_gemm3.h)
 * is bit-identical to the reference arithmetic.  It allocates a small device buffer and SYNCHRONISES the
 * handle's stream: a build-time call (freeze), never on the per-batch path.  w / bias / dy_ch must outlive
 * the plan.  The *_planned entry points are drop-ins for the unplanned ones above (same results bit for bit);
 * shapes or constants outside the pipelined kernel's contract run on the launch-per-tile kernels.          */
typedef struct ivit_linear_plan_s *ivit_linear_plan;
int ivit_linear_plan_create(ivit_handle h, const int8_t *w, const int32_t *bias, const ivit_dyadic *dy_ch, int N, int K,
                            ivit_linear_plan *out);
int ivit_linear_plan_destroy(ivit_linear_plan p);
/* pipelined_ok: the persistent kernel may be used; single_fma_ok: its one-FMA requant form is exact.        */
int ivit_linear_plan_query(ivit_linear_plan p, int *pipelined_ok, int *single_fma_ok);
/* Alignment: x and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant_planned(ivit_handle h, ivit_linear_plan p, const int8_t *x, int bits, void *out, int M);
/* Alignment: x, residual and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x or residual: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant_residual_planned(ivit_handle h, ivit_linear_plan p, const int8_t *x, ivit_dyadic dy_main,
                                            ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int M);
/* Alignment: x, q, k and vt 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: q, k and vt may overlap neither x nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_qkv_planned(ivit_handle h, ivit_linear_plan p, const int8_t *x, int8_t *q, int8_t *k, int8_t *vt,
                               int B, int T, int H, int dh, int ldv);
/* Round 6: K = 384 layers on the kernel that keeps a CU's tokens in LDS and a 64-channel slab of weights in registers
 * (csrc/ivit_gemm_ws.h).  ivit_linear_plan_prepare_ws adds the weights in that kernel's fragment order to a plan (K = 384, N a
 * multiple of 64 up to 1536; IVIT_ERR_UNSUPPORTED otherwise; idempotent; build-time call, synchronises the handle's stream).
 * On a prepared plan ivit_linear_i8_qkv_planned(ldv = 0, dh = 64) and ivit_linear_i8_requant_residual_planned (multipliers in the
 * fast range) run on it — same bytes as on an unprepared plan.
 * ivit_layernorm_linear_i8_qkv_planned = norm1 + qact1 + attn.qkv of a block in ONE launch (vit_quant.py:136-137, 65-74;
 * quant_modules.py:353-386 + quant_utils.py:213-253 + quant_modules.py:21-80): x16 [B*T, 384] is the block's 16-bit input with
 * per-tensor `scale`, bias_int / sc / ln_dy are ivit_layernorm_requant's arguments for norm1, q / k / v are [B*H, T, 64] each
 * (v ROW-major, the ldv = 0 layout).  The bytes are those of ivit_layernorm_requant followed by ivit_linear_i8_qkv_planned;
 * norm1's 8-bit output never exists in HBM.  IVIT_ERR_UNSUPPORTED (nothing launched) unless the plan is prepared, dh = 64 and
 * B*H*T*64 < 2^31.                                                                                             */
int ivit_linear_plan_prepare_ws(ivit_handle h, ivit_linear_plan p);
/* IntLayerNorm + QuantAct(8) + QuantLinear + QuantAct(8) in one launch, plain [M, N] output (swin_quant.py:256-258 + 121-130: norm1 -> qact1 -> attn.qkv of a
 * C = 384 block, activations in natural token order): out8 == ivit_layernorm_requant followed by ivit_linear_i8_requant_planned(bits = 8).
 * IVIT_ERR_UNSUPPORTED (nothing launched) unless the plan is a prepared K = 384 one.  On a prepared plan
 * ivit_linear_i8_requant_planned(bits = 8) runs on the same kernel.                                                            */
/* Alignment: x16 and out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x16: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_linear_i8_requant_planned(ivit_handle h, ivit_linear_plan p, const int16_t *x16, float scale,
                                             const float *bias_int, const float *sc, const ivit_dyadic *ln_dy, int8_t *out8, int M);
/* attn.proj + qact2 with the identity branch + norm2 + qact3 of a D = 384 block in ONE launch (vit_quant.py:137-140):
 * out [M, 384] = ivit_linear_i8_requant_residual_planned's result, ln_out8 [M, 384] = ivit_layernorm_requant(out, ln_scale,
 * ln_bias_int, ln_sc, ln_dy) — the workgroup that produced a row normalises it.  IVIT_ERR_UNSUPPORTED (nothing launched) unless
 * the plan is a prepared 384 x 384 one and both residual multipliers are in the fast range (|m * 2^-e| < 2^9).  Measured SLOWER
 * than the two launches in the DeiT-S forward (profiles/README.md, round 6): the native runner does not use it.            */
/* Alignment: x, residual, out and ln_out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out and ln_out8 may overlap neither x and residual nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant_residual_layernorm_planned(ivit_handle h, ivit_linear_plan p, const int8_t *x, ivit_dyadic dy_main,
                                                      ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int M,
                                                      float ln_scale, const float *ln_bias_int, const float *ln_sc,
                                                      const ivit_dyadic *ln_dy, int8_t *ln_out8);
/* Alignment: x16, q, k and v 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: q, k and v may overlap neither x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_linear_i8_qkv_planned(ivit_handle h, ivit_linear_plan p, const int16_t *x16, float scale,
                                         const float *bias_int, const float *sc, const ivit_dyadic *ln_dy, int8_t *q,
                                         int8_t *k, int8_t *v, int B, int T, int H, int dh);
/* Width 192 (DeiT-Tiny, Swin stage 1): ivit_linear_plan_prepare_ws also takes K = 192, and a prepared K = 192 plan is accepted wherever a
 * prepared K = 384 one is, except by ivit_linear_i8_requant_residual_layernorm_planned.  At K = 192 the kernel also has a v^T store form:
 * ivit_linear_i8_qkv_planned with ldv >= T, ldv % 16 == 0 runs on it, and so does
 * ivit_layernorm_linear_i8_qkv_ldv_planned = ivit_layernorm_linear_i8_qkv_planned with the layout of v as an argument: ldv == 0 is that
 * entry; ldv >= T with ldv % 16 == 0 stores v TRANSPOSED, element (b, h, t, ch) at vt[((b * H + h) * 64 + ch) * ldv + t], the layout of
 * ivit_linear_i8_qkv.  Columns t >= T of v^T are not written.  IVIT_ERR_UNSUPPORTED (nothing launched) where the ldv == 0 entry returns
 * it, and for v^T on a K = 384 plan or with B*H*64*ldv >= 2^31.                                                               */
/* Alignment: x16, q, k and vt 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: q, k and vt may overlap neither x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_linear_i8_qkv_ldv_planned(ivit_handle h, ivit_linear_plan p, const int16_t *x16, float scale,
                                             const float *bias_int, const float *sc, const ivit_dyadic *ln_dy, int8_t *q,
                                             int8_t *k, int8_t *vt, int B, int T, int H, int dh, int ldv);

/* ---- a2  QuantMatMul.forward  (quant_modules.py:223-228), batched, "NT" form:
 * C[b] = A[b] (M x K) * B[b]^T (B[b] is N x K), int32.  q·kᵀ: A=q, B=k.
 * lda/ldb/ldc in elements, strides per batch in elements; lda,ldb % 16 == 0.
 * The four batched products below take at most 65535 matrices per call (nb, BH, B * H: one gridDim.y each); more is
 * IVIT_ERR_UNSUPPORTED, nothing launched.                                                */
/* Alignment: A and B 16-byte aligned; C takes any int32 address; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: C may not overlap A or B: IVIT_ERR_INVALID, nothing launched. */
int ivit_bmm_nt_i8(ivit_handle h, const int8_t *A, const int8_t *B, int32_t *C, int nb, int M,
                   int N, int K, int lda, int ldb, int ldc, int64_t strideA, int64_t strideB,
                   int64_t strideC);
/* attn·v with the 16-bit Shiftmax output as A (values 0..32768): exact, two int8 MFMA
 * passes (a-16384 = 256*hi + lo) + 16384*colsum(B).  B = vᵀ [N=dh, K=T].                */
/* Alignment: A and B 16-byte aligned; C takes any int32 address; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: C may not overlap A or B: IVIT_ERR_INVALID, nothing launched. */
int ivit_bmm_nt_u16i8(ivit_handle h, const uint16_t *A, const int8_t *B, int32_t *C, int nb,
                      int M, int N, int K, int lda, int ldb, int ldc, int64_t strideA,
                      int64_t strideB, int64_t strideC);

/* a2 + a3, attention-shaped (vit_quant.py:70-74, 79-83):
 * scores8[bh,i,j] = clamp8(rq(q[bh,i,:]·k[bh,j,:], dy));  scores8 is [B*H, T, lds]; columns j >= T of a row are not written. */
/* Alignment: q, k and scores8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: scores8 may not overlap q or k: IVIT_ERR_INVALID, nothing launched. */
int ivit_attn_qk_requant(ivit_handle h, const int8_t *q, const int8_t *k, ivit_dyadic dy,
                         int8_t *scores8, int BH, int T, int dh, int lds);
/* ctx8[b,i,h*dh+d] = clamp8(rq(sum_j p[bh,i,j]*v[bh,j,d], dy));  p is [B*H,T,ldp] uint16,
 * vt is [B*H,dh,ldv];  ctx8 is [B,T,H*dh] (heads merged, vit_quant.py:81).               */
/* Alignment: p, vt and ctx8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx8 may not overlap p or vt: IVIT_ERR_INVALID, nothing launched. */
int ivit_attn_pv_requant(ivit_handle h, const uint16_t *p, const int8_t *vt, ivit_dyadic dy,
                         int8_t *ctx8, int B, int H, int T, int dh, int ldp, int ldv);

/* a10 core, fused (vit_quant.py:70-83): matmul_1 -> *scale -> qact_attn1 -> IntSoftmax(16)
 * -> matmul_2 -> qact2 in ONE kernel per (image, head); scores and probabilities stay in
 * registers.  Bit-identical to ivit_attn_qk_requant + ivit_shiftmax + ivit_attn_pv_requant.
 * q,k [B*H,T,dh], vt [B*H,dh,ldv] (as written by ivit_linear_i8_qkv), ctx8 [B,T,H*dh].
 * Built for dh == 64 and T <= 640 (DeiT/ViT at 224 and 384); else IVIT_ERR_UNSUPPORTED.   */
/* Alignment: q, k, vt and ctx8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx8 may not overlap q, k or vt: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                         ivit_dyadic dy_qk, float s_softmax, ivit_dyadic dy_pv, int8_t *ctx8,
                         int B, int H, int T, int dh, int ldv);

/* The same with Shiftmax's exp_int taken from tables built on the host for the layer's frozen scale
 * (ivit_amd.freeze.shiftmax_tables; exhaustively checked against the arithmetic form when built):
 * exp_int = exp_t[exp_aq[exp_cls[vmax]][v] + max(v - vmax, dmin) - dmin].  exp_aq uint16 [nclass][256],
 * exp_t float [t_count], exp_cls uint8 [256] (device; exp_aq and exp_t 16-byte aligned, exp_cls 4-byte aligned — they are
 * copied into LDS in 16-byte pieces; IVIT_ERR_INVALID otherwise).  Same integers as ivit_attention_fused.        */
/* Alignment: q, k, vt and ctx8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx8 may not overlap q, k or vt: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused_lut(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                             ivit_dyadic dy_qk, float s_softmax, const uint16_t *exp_aq, const float *exp_t,
                             const uint8_t *exp_cls, int nclass, int t_count, int dmin, ivit_dyadic dy_pv,
                             int8_t *ctx8, int B, int H, int T, int dh, int ldv);

/* Row form of the same tables (round 6).  In a score row with maximum vmax only the scores v in (vmax + dmin, vmax] have an
 * exp_int above the floor constant (IntSoftmax.int_exp_shift, quant_modules.py:469-481), so exp_int as a function of
 * dd = max(v - vmax, dmin) - dmin is ONE line of R = 1 - dmin entries per value of vmax:
 *     rowtab[vmax + 128][dd] = exp_t[exp_aq[exp_cls[vmax]][vmax + dmin + dd] + dd],   float [256][64] (device, 16-byte aligned).
 * ivit_shiftmax_rowtable builds it on the device from the tables of ivit_attention_fused_lut (IVIT_ERR_UNSUPPORTED when a
 * line does not fit: 1 - dmin > 64; the two-level form then stays); ivit_attention_fused_rowlut is ivit_attention_fused with
 * ONE table gather per score: a wavefront fetches the 16 lines of its query tile once the row maxima are known.  Needs
 * |m 2^-e| < 2^9 for both requant multipliers (IVIT_ERR_UNSUPPORTED otherwise).  Same integers as ivit_attention_fused
 * (vit_quant.py:70-83).
 * ldv == 0 (this entry point only): `vt` is v ROW-major [B*H, T, dh] — what ivit_linear_i8_qkv / _planned write when THEIR ldv is 0
 * (one 16-byte store per token and head instead of sixteen byte stores); the kernel transposes on its way into the LDS.      */
int ivit_shiftmax_rowtable(ivit_handle h, const uint16_t *exp_aq, const float *exp_t, const uint8_t *exp_cls,
                           int nclass, int t_count, int dmin, float *rowtab);
/* Alignment: q, k, vt and ctx8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx8 may not overlap q, k or vt: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused_rowlut(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                ivit_dyadic dy_qk, float s_softmax, const float *rowtab, int dmin, ivit_dyadic dy_pv,
                                int8_t *ctx8, int B, int H, int T, int dh, int ldv);

/* Class-token forms of the three entries above (vit_quant.py:70-83 for query row 0 of every image; the head, vit_quant.py:271-281,
 * reads that row alone).  A context row depends on its own q row and on k and v of all tokens: K and V are staged as in the whole-T
 * form and one query tile is worked.  ctx_cls int8 [B, H*dh] receives what the whole-T entry writes to rows b*T of ctx8, the same
 * integers.  x16 / x_cls (both NULL: skipped): row b*T of the 16-bit stream x16 [B*T, H*dh] is copied to x_cls [B, H*dh] on the side
 * — the identity rows of the attn.proj that follows (vit_quant.py:135).  ctx_cls, x16 and x_cls 16-byte aligned; otherwise the
 * arguments, limits and status codes of the whole-T entry of the same Shiftmax form.                                               */
/* Alignment: q, k and vt 16-byte aligned, like ctx_cls, x16 and x_cls; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx_cls and x_cls may overlap neither q, k, vt and x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                             ivit_dyadic dy_qk, float s_softmax, ivit_dyadic dy_pv, int8_t *ctx_cls,
                             const int16_t *x16, int16_t *x_cls, int B, int H, int T, int dh, int ldv);
/* Alignment: q, k and vt 16-byte aligned, like ctx_cls, x16 and x_cls; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx_cls and x_cls may overlap neither q, k, vt and x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused_lut_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                 ivit_dyadic dy_qk, float s_softmax, const uint16_t *exp_aq, const float *exp_t,
                                 const uint8_t *exp_cls, int nclass, int t_count, int dmin, ivit_dyadic dy_pv,
                                 int8_t *ctx_cls, const int16_t *x16, int16_t *x_cls, int B, int H, int T, int dh, int ldv);
/* Alignment: q, k and vt 16-byte aligned, like ctx_cls, x16 and x_cls; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx_cls and x_cls may overlap neither q, k, vt and x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_attention_fused_rowlut_cls(ivit_handle h, const int8_t *q, const int8_t *k, const int8_t *vt,
                                    ivit_dyadic dy_qk, float s_softmax, const float *rowtab, int dmin, ivit_dyadic dy_pv,
                                    int8_t *ctx_cls, const int16_t *x16, int16_t *x_cls, int B, int H, int T, int dh, int ldv);
/* out[r, :] = x[r * row_stride : r * row_stride + C] for r < rows (16-bit values; x[:, 0] of vit_quant.py:272 with
 * row_stride = T * C): the identity-row copy above as a launch of its own.  C and row_stride multiples of 8, 16-byte aligned.    */
/* Alignment: x and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_gather_rows_i16(ivit_handle h, const int16_t *x, int64_t rows, int C, int64_t row_stride, int16_t *out);

/* ---- a3  QuantAct.forward with a previous scale -> fixedpoint_mul.forward
 * (quant_modules.py:197-206, quant_utils.py:192-253).  z int32 or float (integer-valued;
 * the I-LayerNorm output exceeds int32), [rows, C];  dy has nch = 1 or C entries;
 * optional identity z_id (int32, same shape) with scalar dy_id;  bits 8 -> int8 out,
 * 16 -> int16 out, 32 -> int32 out.                                                      */
/* Overlap: out may not overlap z or z_id: IVIT_ERR_INVALID, nothing launched. */
int ivit_requant_i32(ivit_handle h, const int32_t *z, const ivit_dyadic *dy, int nch,
                     const int32_t *z_id, const ivit_dyadic *dy_id, int bits, void *out,
                     int64_t rows, int C);
/* Overlap: out may not overlap z or z_id: IVIT_ERR_INVALID, nothing launched. */
int ivit_requant_i16(ivit_handle h, const int16_t *z, const ivit_dyadic *dy, int nch,
                     const int32_t *z_id, const ivit_dyadic *dy_id, int bits, void *out,
                     int64_t rows, int C);
/* Overlap: out may not overlap z or z_id: IVIT_ERR_INVALID, nothing launched. */
int ivit_requant_f32(ivit_handle h, const float *z, const ivit_dyadic *dy, int nch,
                     const int32_t *z_id, const ivit_dyadic *dy_id, int bits, void *out,
                     int64_t rows, int C);

/* ---- a5  IntSoftmax.forward (Shiftmax)  (quant_modules.py:469-497).
 * x int8 [rows, n] (row stride ld_in), per-tensor scale; out_bits 16 (ViT/DeiT) or 8 (Swin);
 * integer probabilities with scale 2^-(out_bits-1), stored uint16 (16-bit results reach
 * 32768).  fp32-faithful interior incl. torch's CPU summation order.                     */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_shiftmax(ivit_handle h, const int8_t *x, int64_t rows, int n, int ld_in, float scale,
                  int out_bits, uint16_t *out, int ld_out);

/* ---- a6  IntGELU.forward (ShiftGELU)  (quant_modules.py:410-445).
 * x int8 [rows, C], per-tensor scale -> out16[i] = Q*sigmoid_int (scale s*2^-7).
 * Scale domain: sigmoid_int <= 256 and the product fits 16 bits only while the reference's clamp of the
 * exponential sum at 2^31 (:437) does not bite, i.e. for scales above about 1.2e-3.  The entry point
 * evaluates the extremes of Q*sigmoid_int over all (Q, row max) pairs on the host, from the scale alone,
 * and returns IVIT_ERR_UNSUPPORTED (nothing launched, the message names the scale) when they leave int16.
 * The 8-bit forms below carry the product in 32 bits and equal the reference at every positive scale.  */
/* Alignment: x and out16 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out16 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_shiftgelu(ivit_handle h, const int8_t *x, int64_t rows, int C, float scale,
                   int16_t *out16);
/* a6 + a3 (layers_quant.py:146-147): ... -> clamp8(rq(Q*sigmoid_int, dy))               */
/* Alignment: x and out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_shiftgelu_requant(ivit_handle h, const int8_t *x, int64_t rows, int C, float scale,
                           ivit_dyadic dy, int8_t *out8);

/* Same function as ivit_shiftgelu_requant, table form.  For a frozen layer the int8 result
 * depends only on (Q, row max): ivit_shiftgelu_build_table fills table[(qmax+128)*256 +
 * (Q+128)] (65536 bytes) once with the same device arithmetic; the per-token call is then
 * a row max plus byte gathers (HBM-bound instead of VALU-bound).                          */
int ivit_shiftgelu_build_table(ivit_handle h, float scale, ivit_dyadic dy, int8_t *table);
/* Alignment: x and out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_shiftgelu_requant_lut(ivit_handle h, const int8_t *x, int64_t rows, int C,
                               const int8_t *table, int8_t *out8);

/* ---- a7  IntLayerNorm.forward  (quant_modules.py:353-386).
 * x int16 [rows, C] with per-tensor scale; bias_int[c] = floor(fl(fl(b/w)/sf)) and
 * sc[c] = fl(sf*w[c]) from the host.  z[i,c] = rne(fl(fl(out*sc)/sc)) as float — the
 * integer the following QuantAct derives (quant_utils.py:220).                           */
/* Alignment: x and z 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: z may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale,
                   const float *bias_int, const float *sc, float *z);
/* a7 + a3 (vit_quant.py:131-132): ... -> clamp8(rq(z, dy_ch[c])).  row_stride in
 * elements lets the final norm read only the class-token rows (vit_quant.py:271-272).    */
/* Alignment: x and out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_requant(ivit_handle h, const int16_t *x, int64_t rows, int C,
                           int64_t row_stride, float scale, const float *bias_int,
                           const float *sc, const ivit_dyadic *dy_ch, int8_t *out8);

/* ---- a8  PatchEmbed.forward: QuantConv2d(kernel=stride=P) -> QuantAct(16)
 * (layers_quant.py:184-196, quant_modules.py:297-330), then class token + position
 * embedding (vit_quant.py:259-265).
 * ivit_im2col_patch: NCHW int8 image -> [B*gh*gw, Cin*P*P] rows in conv-weight order, any B
 * (B * gh is its grid beyond 65535 images).  ivit_embed_finish and ivit_patch_embed take B <= 65535 (an image is one
 * gridDim.y): IVIT_ERR_INVALID / IVIT_ERR_UNSUPPORTED beyond, nothing launched.           */
/* Alignment: img and rows 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: rows may not overlap img: IVIT_ERR_INVALID, nothing launched. */
int ivit_im2col_patch(ivit_handle h, const int8_t *img, int B, int Cin, int H, int W, int P,
                      int8_t *rows);
/* x16[b,0,:]  = clamp16(rq(z_cls[:], dy_x) + rq(pos[0,:], dy_pos))
 * x16[b,1+i,:] = clamp16(rq(patch16[b,i,:], dy_x) + rq(pos[1+i,:], dy_pos))             */
/* Alignment: patch16 and x16 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: x16 may not overlap patch16: IVIT_ERR_INVALID, nothing launched. */
int ivit_embed_finish(ivit_handle h, const int16_t *patch16, const int32_t *z_cls,
                      const int16_t *pos, ivit_dyadic dy_x, ivit_dyadic dy_pos, int16_t *x16,
                      int B, int T, int D);
/* Round 6: the three steps above in one GEMM launch (plus the B class-token rows): the A rows are gathered from the NCHW images
 * (every 16-byte chunk of an im2col row is one pixel row of a 16 x 16 patch), the epilogue requantises to 16 bits, adds the
 * patch's position embedding and writes row 1 + i of its image.  w [D, Cin*P*P] in conv-weight order, bias int32 [D] or NULL,
 * dy_ch [D] as for ivit_linear_i8_requant(bits = 16).  x16 == ivit_im2col_patch -> ivit_linear_i8_requant(16) -> ivit_embed_finish.
 * IVIT_ERR_UNSUPPORTED (nothing launched) unless P == 16, H and W multiples of 16, Cin*P*P a multiple of 64 and |dy_x|, |dy_pos| < 2^9. */
/* Alignment: images and x16 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: x16 may not overlap images: IVIT_ERR_INVALID, nothing launched. */
int ivit_patch_embed(ivit_handle h, const int8_t *images, int B, int Cin, int H, int W, int P, const int8_t *w,
                     const int32_t *bias, const ivit_dyadic *dy_ch, const int32_t *z_cls, const int16_t *pos,
                     ivit_dyadic dy_x, ivit_dyadic dy_pos, int16_t *x16, int D);

/* ---- a9-a11  whole-model runner: VisionTransformer.forward (vit_quant.py:254-282) with
 * Block.forward (:130-143), Attention.forward (:59-88) and Mlp.forward (layers_quant.py:144-153)
 * chained natively.  Replaces the Python module tree for inference on frozen constants: one C call
 * per batch, nothing allocated after ivit_vit_create, the whole forward capturable in a hipGraph.
 *
 * All `const T *` members point into DEVICE memory owned by the caller (typically one packed blob
 * that was broadcast once over RCCL); scalars and by-value dyadics are host values.            */
typedef struct ivit_vit_config {
    int img_size, patch_size, in_chans, embed_dim, depth, num_heads, hidden_dim, num_classes;
} ivit_vit_config;

typedef struct ivit_vit_block {
    /* norm1 -> qact1 (vit_quant.py:131-132) */
    float s_ln1; const float *n1_bias_int; const float *n1_sc; const ivit_dyadic *n1_dy;
    /* attn.qkv -> qact1 (:63-65); q.k^T*scale -> qact_attn1 (:71-73); Shiftmax (:74);
       attn.v -> qact2 (:77-79); proj -> qact3 (:80-82) */
    const int8_t *qkv_w; const int32_t *qkv_b; const ivit_dyadic *qkv_dy;
    ivit_dyadic dy_qk; float s_softmax; ivit_dyadic dy_pv;
    const uint16_t *exp_aq; const float *exp_t; const uint8_t *exp_cls;   /* optional Shiftmax tables (NULL: arithmetic) */
    int exp_nc, exp_tcount, exp_dmin;
    const int8_t *proj_w; const int32_t *proj_b; const ivit_dyadic *proj_dy;
    ivit_dyadic res1_main, res1_res;                       /* qact2 with identity (:134) */
    /* norm2 -> qact3 (:135-136); mlp (layers_quant.py:144-153); qact4 with identity (:138) */
    float s_ln2; const float *n2_bias_int; const float *n2_sc; const ivit_dyadic *n2_dy;
    const int8_t *fc1_w; const int32_t *fc1_b; const ivit_dyadic *fc1_dy;
    float s_gelu; ivit_dyadic dy_gelu;
    const int8_t *fc2_w; const int32_t *fc2_b; const ivit_dyadic *fc2_dy;
    ivit_dyadic res2_main, res2_res;
} ivit_vit_block;

typedef struct ivit_vit_params {
    const int8_t *pe_w; const int32_t *pe_b; const ivit_dyadic *pe_dy;   /* patch_embed.proj -> qact */
    const int32_t *z_cls; const int16_t *pos; ivit_dyadic dy_x, dy_pos;  /* cls token, pos_embed, qact1 */
    const ivit_vit_block *blocks_host;                                   /* HOST array [depth]        */
    float s_ln; const float *n_bias_int; const float *n_sc; const ivit_dyadic *n_dy;   /* norm -> qact2 */
    const int8_t *head_w; const int32_t *head_b;                         /* head (int32 accumulators) */
} ivit_vit_params;

typedef struct ivit_vit_s *ivit_vit;

/* Builds the per-layer ShiftGELU tables (device allocation happens here, never later) and
 * `max_slices` internal streams/events for the sliced mode.                                     */
int ivit_vit_create(ivit_handle h, const ivit_vit_config *cfg, const ivit_vit_params *params,
                    int max_slices, ivit_vit *out);
int ivit_vit_destroy(ivit_vit m);
/* Caller-provided workspace: bytes for `batch` images cut into `nslices` slices.               */
int ivit_vit_workspace_bytes(ivit_vit m, int batch, int nslices, size_t *bytes);
/* How many blocks of a forward of `batch` images in ONE slice issue their Mlp as a single launch (the fused kernels of
 * ivit_mlp_plan_create); the other blocks run fc1 / ShiftGELU / fc2 as three.  Decided by the rule the forward itself applies. */
int ivit_vit_fused_mlp_blocks(ivit_vit m, int batch, int *blocks);
/* How many blocks of a forward of `batch` images in ONE slice issue norm2 + qact3 + the Mlp + the residual QuantAct as a single launch,
 * through either LayerNorm-headed entry (ivit_layernorm_mlp_fused_planned, ivit_layernorm_mlp_lockstep_planned); the other blocks run
 * the LayerNorm as a launch of its own.  The last block is counted at the row count of its class-token tail (ivit_vit_cls_tail).
 * Decided by the rule the forward itself applies.                                                                                */
int ivit_vit_fused_ln_mlp_blocks(ivit_vit m, int batch, int *blocks);
/* How many blocks of a forward of `batch` images in ONE slice issue norm1 + qact1 + attn.qkv as a single launch
 * (ivit_layernorm_linear_i8_qkv_ldv_planned: D = 192 or 384 with dh = 64; a D = 384 block only where it takes v row-major); the other
 * blocks run the LayerNorm and the GEMM as two.  Decided by the rule the forward itself applies.                               */
int ivit_vit_fused_qkv_blocks(ivit_vit m, int batch, int *blocks);
/* *on = 1 when a forward of `batch` images runs the last block's attention, attn.proj, norm2 and Mlp on the class-token rows only
 * (B rows instead of B*T; the head reads no other row, vit_quant.py:271-281): models on the fused attention (dh == 64, T <= 640).
 * Same logits either way.  Decided by the rule the forward itself applies.                                                      */
int ivit_vit_cls_tail(ivit_vit m, int batch, int *on);
/* Must run once per (workspace, batch, nslices) before the first forward (zeroes the padded
 * key columns of the transposed V buffers); asynchronous on the handle's stream.               */
int ivit_vit_workspace_init(ivit_vit m, void *workspace, size_t bytes, int batch, int nslices);
/* images int8 [batch, in_chans, img, img] -> logits int32 [batch, num_classes].
 * nslices == 1: everything on the handle's stream.  nslices > 1: the batch is cut into slices that
 * run on internal streams forked from / joined to the handle's stream with events, so VALU-bound
 * kernels of one slice overlap MFMA-bound GEMMs of another.  Same integers either way.
 * A slice holds at most 65535 images (an image is one gridDim.y of the embedding launches), and at most 65535 / num_heads where the
 * model does not run the fused attention (head dim != 64 or more than 640 tokens: an (image, head) is one matrix of the batched
 * products).  A forward, and every runner entry with a forward in it, whose largest slice ceil(batch / nslices) is larger returns
 * IVIT_ERR_UNSUPPORTED before anything is launched, with "images per slice" and the limit in ivit_last_error: use more slices.
 * ivit_swin_forward has no such limit.                                                          */
int ivit_vit_forward(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace,
                     size_t bytes, int32_t *logits);
/* hipGraph of one ivit_vit_forward call with fixed buffers; launch replays it on the handle's
 * stream.                                                                                      */
typedef struct ivit_graph_s *ivit_graph;
int ivit_vit_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace,
                          size_t bytes, int32_t *logits, ivit_graph *out);
int ivit_graph_launch(ivit_graph g);
int ivit_graph_destroy(ivit_graph g);

/* ---- a12  whole-model runner for Swin: SwinTransformer.forward (swin_quant.py:539-564) with
 * SwinTransformerBlock.forward (:251-301), WindowAttention.forward (:121-169), PatchMerging.forward
 * (:328-349) and PatchEmbed.forward (layers_quant.py:184-196) chained natively; activations stay in natural
 * token order, roll / window partition / reverse are index arithmetic inside ivit_window_attention_fused.
 * Built for window 7 (every reference factory) or 12 (patch4_window12_384), head dim 32; a stage whose
 * resolution is at most the window runs one window of that resolution, unshifted (SwinTransformerBlock).
 * Same conventions as ivit_vit_*.                                                               */
typedef struct ivit_ln_params { const float *bias_int; const float *sc; const ivit_dyadic *dy; } ivit_ln_params;
typedef struct ivit_lin_params { const int8_t *w; const int32_t *b; const ivit_dyadic *dy; } ivit_lin_params;

typedef struct ivit_swin_config {
    int img_size, patch_size, in_chans, embed_dim, num_layers, window_size, mlp_ratio, num_classes;
    int depths[4];
    int num_heads[4];
} ivit_swin_config;

typedef struct ivit_swin_block {
    float s_in; ivit_ln_params n1;                         /* norm1 -> qact1 (:253-255)                         */
    ivit_lin_params qkv;                                   /* attn.qkv -> attn.qact1 (:123-124)                 */
    ivit_dyadic dy_qk, dy_a; const int16_t *relb;          /* qact_attn1; qact2 with the bias identity (:133-149) */
    float s_softmax; ivit_dyadic dy_pv;                    /* Shiftmax 8 bit (:151-157); attn.v -> qact3 (:159-162) */
    ivit_lin_params proj;                                  /* attn.proj -> attn.qact4 (:163-164)                */
    ivit_dyadic res1_main, res1_res;                       /* qact2 with identity (:289)                        */
    float s_mid; ivit_ln_params n2;                        /* norm2 -> qact3 (:291-292)                         */
    ivit_lin_params fc1; float s_gelu; ivit_dyadic dy_gelu; ivit_lin_params fc2;   /* mlp (layers_quant.py:144-153) */
    ivit_dyadic res2_main, res2_res;                       /* qact4 with identity (:296)                        */
    const uint16_t *exp_aq; const float *exp_t; const uint8_t *exp_cls;   /* optional Shiftmax tables for s_softmax (NULL: arithmetic) */
    int exp_nc, exp_tcount, exp_dmin;                      /* zero-initialise the struct: garbage here is read as pointers */
} ivit_swin_block;

typedef struct ivit_swin_merge {                           /* PatchMerging: norm -> qact1 -> reduction -> qact2 */
    float s_in; ivit_ln_params n; ivit_lin_params red;
} ivit_swin_merge;

typedef struct ivit_swin_params {
    ivit_lin_params pe; float s_bn;                        /* patch_embed.proj -> qact_before_norm (8 bit)      */
    ivit_ln_params pn; const ivit_dyadic *dy_qact1;        /* patch_embed.norm -> qact (16); qact1 (16), 1 entry */
    const ivit_swin_block *blocks_host;                    /* HOST array [sum(depths)], stage-major             */
    const ivit_swin_merge *merges_host;                    /* HOST array [num_layers - 1]                       */
    float s_norm_in; ivit_ln_params n;                     /* norm -> qact2                                     */
    ivit_dyadic dy_pool;                                   /* avgpool -> qact3                                  */
    const int8_t *head_w; const int32_t *head_b;
    float s_pool;                                          /* qact2 scale: the pool's input (even token counts) */
} ivit_swin_params;

typedef struct ivit_swin_s *ivit_swin;
int ivit_swin_create(ivit_handle h, const ivit_swin_config *cfg, const ivit_swin_params *params,
                     int max_slices, ivit_swin *out);
int ivit_swin_destroy(ivit_swin m);
int ivit_swin_workspace_bytes(ivit_swin m, int batch, int nslices, size_t *bytes);
/* Per stage: how many blocks of a forward of `batch` images in ONE slice issue their Mlp as a single launch (ivit_mlp_fused in
 * the C = 96 / C = 128 stage, ivit_mlp_fused_planned in the C = 192, C = 256 and C = 384 stages).  Decided by the rule the forward itself applies;
 * stages the model does not have report 0.                                                                             */
int ivit_swin_fused_mlp_blocks(ivit_swin m, int batch, int blocks_per_stage[4]);
int ivit_swin_forward(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace,
                      size_t bytes, int32_t *logits);
int ivit_swin_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace,
                           size_t bytes, int32_t *logits, ivit_graph *out);

/* ---- a12  Swin-specific operators (models/swin_quant.py)
 * IntSoftmax on `attn + mask` (:151-156): float mask [nW, n, n] (0 / -100.0) added to fl(Q*s)
 * before the division by s; row r of the flattened [B_, H, n] rows uses window (r/(H*n)) % nW.
 * mask == NULL: identical to ivit_shiftmax.                                                */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_shiftmax_masked(ivit_handle h, const int8_t *x, int64_t rows, int n, int ld_in, float scale,
                         int out_bits, const float *mask, int nW, int H, uint16_t *out, int ld_out);
/* QuantAct with an identity that repeats every id_period elements (relative position bias
 * [H,N,N] broadcast over windows, :149): out = clamp(rq(z[i],dy) + rq(z_id[i % period],dy_id)) */
/* Overlap: out may not overlap z: IVIT_ERR_INVALID, nothing launched. */
int ivit_requant_i32_bcast(ivit_handle h, const int32_t *z, ivit_dyadic dy, const int32_t *z_id,
                           int64_t id_period, ivit_dyadic dy_id, int bits, void *out, int64_t total);
/* AdaptiveAvgPool1d(1) over L (odd) tokens + QuantAct(8) (:553-555): x int8 [B,L,C] -> [B,C]   */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_avgpool_requant(ivit_handle h, const int8_t *x, int B, int L, int C, ivit_dyadic dy,
                         int8_t *out8);
/* The same for any L, given the input scale: with L even rounding ties are reachable and are
 * decided by the reference's fp32 sequence (fl(Q*s), torch's token-sum order, fl(sum/L),
 * rint(fl(mean/s))), restated exactly; odd L gives the outputs of ivit_avgpool_requant.      */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_avgpool_requant_scaled(ivit_handle h, const int8_t *x, int B, int L, int C, float scale,
                                ivit_dyadic dy, int8_t *out8);
/* IntLayerNorm whose row sums follow torch's order for a TOKEN-contiguous input — what the
 * reference computes in Swin stage 0, where activations keep the layout of
 * flatten(2).transpose(1,2) (layers_quant.py:188).  Same outputs as
 * ivit_layernorm otherwise.                                                                */
/* Overlap: z may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_tokenorder(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale,
                              const float *bias_int, const float *sc, int tokens_per_image, float *z);

/* the same with the per-channel QuantAct(8) that follows fused in (out8 int8 [rows, C]).  For C = 96 / 128 (the
 * vectorised kernel) x, out8, bias_int and sc must be 16-byte aligned: IVIT_ERR_INVALID otherwise; the same holds for
 * ivit_patch_norm_tokenorder below.                                                              */
/* Alignment: at C = 96 / 128 x and out8 16-byte aligned (the other widths take any element-aligned address); IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_tokenorder_requant(ivit_handle h, const int16_t *x, int64_t rows, int C, float scale,
                                      const float *bias_int, const float *sc, const ivit_dyadic *dy,
                                      int tokens_per_image, int8_t *out8);
/* PatchEmbed's tail in one pass (layers_quant.py:193-195, swin_quant.py:543): int8 conv output ->
 * norm (token-order sums) -> qact (16 bit, per-channel dy_ch) -> qact1 (16 bit, per-tensor dy2).          */
/* Alignment: at C = 96 / 128 x8 and out16 16-byte aligned (the other widths take any element-aligned address); IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out16 may not overlap x8: IVIT_ERR_INVALID, nothing launched. */
int ivit_patch_norm_tokenorder(ivit_handle h, const int8_t *x8, int64_t rows, int C, float scale,
                               const float *bias_int, const float *sc, const ivit_dyadic *dy_ch,
                               ivit_dyadic dy2, int tokens_per_image, int16_t *out16);
/* Fused windowed attention: everything of WindowAttention.forward (swin_quant.py:121-169) between
 * the qkv QuantAct and proj — q.k^T*scale -> qact_attn1 -> (+ relative position bias) qact2 ->
 * Shiftmax 8 bit on attn (+ shift mask, :151-156) -> attn.v -> qact3 — including torch.roll,
 * window_partition and their inverses (swin_quant.py:18-50, 268-287) as index arithmetic.
 * qkv int8 [B, R, R, 3, heads, dh] in natural token order; ctx int8 [B, R*R, heads*dh] natural order.
 * relb int16 [heads, N, N] (N = window^2) = rq(quantised bias table gathered by
 * relative_position_index, dy(qact_table -> qact2)); dy_a = dy(qact_attn1 -> qact2).
 * Built for window 7 (R % 7 == 0) and window 12 (R % 12 == 0, relb 16-byte aligned), dh 32.  */
/* Alignment: qkv and ctx 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx may not overlap qkv: IVIT_ERR_INVALID, nothing launched. */
int ivit_window_attention_fused(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a,
                                const int16_t *relb, float s_softmax, ivit_dyadic dy_pv, int8_t *ctx,
                                int B, int R, int window, int shift, int heads, int dh);
/* The same with Shiftmax's exp_int (IntSoftmax.int_exp_shift, quant_modules.py:469-481) taken from the tables of
 * ivit_attention_fused_lut (ivit_amd.freeze.shiftmax_tables for the layer's frozen qact2 scale; same layout, alignment and
 * errors) in the windows that carry no shift mask; windows under the mask (swin_quant.py:151-156) keep the arithmetic
 * form, because the float -100 enters between the requotient's multiply and divide.  Same integers as the entry above.
 * Window 7 only (IVIT_ERR_UNSUPPORTED at window 12).                                                                  */
/* Alignment: qkv and ctx 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: ctx may not overlap qkv: IVIT_ERR_INVALID, nothing launched. */
int ivit_window_attention_fused_lut(ivit_handle h, const int8_t *qkv, ivit_dyadic dy_qk, ivit_dyadic dy_a,
                                    const int16_t *relb, float s_softmax, const uint16_t *exp_aq, const float *exp_t,
                                    const uint8_t *exp_cls, int nclass, int t_count, int dmin, ivit_dyadic dy_pv,
                                    int8_t *ctx, int B, int R, int window, int shift, int heads, int dh);
/* Fused Mlp.forward + closing QuantAct(identity) for a narrow stage (layers_quant.py:144-153,
 * swin_quant.py:293-296): fc1 -> qact_gelu(8) -> ShiftGELU -> qact1(8) -> fc2 -> qact2(16) -> qact4(16, +identity)
 * with the hidden tensor never written to HBM.  Stateless: the operands are the caller's own arrays, nothing is kept between calls.
 * x int8 [M, C] (norm2 -> qact3), gelu_table from ivit_shiftgelu_build_table, residual / out int16 [M, C].
 * Built for C = 96, hidden = 384 (Swin-T/S stage 0: both weight matrices resident in LDS or registers) and for C = 128,
 * hidden = 512 (Swin-B stage 0: the lock-step kernel of csrc/ivit_mlp.h reading w1 / w2 row-major from L2; there x, w1, w2, b1, b2,
 * dy1, dy2 must be 16-byte aligned, and residual multipliers >= 2^9 are IVIT_ERR_UNSUPPORTED with nothing launched);
 * other shapes: IVIT_ERR_UNSUPPORTED.                                                                   */
/* Alignment: x, residual and out 16-byte aligned (C = 128: residual and out 8-byte aligned); IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x or residual (judged at the two shapes the entry is built for, an unsupported shape addresses nothing): IVIT_ERR_INVALID, nothing launched. */
int ivit_mlp_fused(ivit_handle h, const int8_t *x, const int8_t *w1, const int32_t *b1, const ivit_dyadic *dy1,
                   const int8_t *gelu_table, const int8_t *w2, const int32_t *b2, const ivit_dyadic *dy2,
                   ivit_dyadic dy_main, ivit_dyadic dy_res, const int16_t *residual, int16_t *out, int64_t M,
                   int C, int hidden);
/* The same chain on frozen linear plans, at three widths: C = 384, hidden = 1536 (DeiT-S, Swin-T / S stage 2), C = 256,
 * hidden = 1024 (Swin-B stage 1) and C = 192, hidden = 768 (DeiT-Tiny, Swin-T / S stage 1).  Both weight matrices are re-laid-out once in MFMA-fragment order and
 * stream L2 -> registers, the hidden tile of a unit of up to 80 tokens lives in LDS between fc1, the ShiftGELU table pass
 * and fc2 (csrc/ivit_mlp.h: one lock-step kernel body at every width, two four-wave workgroups per CU at width 192; csrc/ivit_mlp_rs.h).  x, residual and out
 * are [M, C] of the plan's width.  The linear plans are borrowed and must outlive the Mlp plan.
 * IVIT_ERR_UNSUPPORTED for other shapes (fc1 must be [4C x C] and fc2 [C x 4C] with C = 384, 256 or 192), for plans whose requant bound is not provable, and (at call time) for
 * residual multipliers >= 2^9: callers then run the unfused chain.  Replaces layers_quant.py:144-153 +
 * vit_quant.py:141-142 (swin_quant.py:296-300) like ivit_mlp_fused.                                        */
typedef struct ivit_mlp_plan_s *ivit_mlp_plan;
int ivit_mlp_plan_create(ivit_handle h, ivit_linear_plan fc1, ivit_linear_plan fc2, ivit_mlp_plan *out);
int ivit_mlp_plan_destroy(ivit_mlp_plan p);
/* Tuning / test switch: which of a width-384 plan's two kernels ivit_mlp_fused_planned launches.  0 = by shape (the default:
 * the role-split kernel of csrc/ivit_mlp_rs.h from two 80-token units per CU on, the lock-step kernel of csrc/ivit_mlp.h
 * below that), 1 = lock-step, 2 = role-split.  Both compute the same integers (layers_quant.py:144-153).  NOT safe to call
 * while another thread or stream is inside ivit_mlp_fused_planned on the same plan: it rewrites a field the launch reads.
 * A width-192 or width-256 plan has the lock-step kernel only: 0 and 1 succeed, 2 returns IVIT_ERR_UNSUPPORTED and changes nothing.  */
int ivit_mlp_plan_select(ivit_mlp_plan p, int kernel);
/* Alignment: x, residual and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x or residual: IVIT_ERR_INVALID, nothing launched. */
int ivit_mlp_fused_planned(ivit_handle h, ivit_mlp_plan p, const int8_t *x, const int8_t *gelu_table,
                           ivit_dyadic dy_main, ivit_dyadic dy_res, const int16_t *residual, int16_t *out,
                           int64_t M);
/* Round 6: norm2 + qact3 + the fused Mlp + the block's residual QuantAct in ONE launch (vit_quant.py:139-142): every workgroup first
 * normalises the rows it is going to multiply (x16 [M, 384], the block's 16-bit stream, which is also the identity branch; scale /
 * bias_int / sc / ln_dy as for ivit_layernorm_requant) into scratch8 [M, 384] and reads its activation tiles from there.  out ==
 * ivit_layernorm_requant followed by ivit_mlp_fused_planned.  IVIT_ERR_UNSUPPORTED (nothing launched) where ivit_mlp_fused_planned is,
 * where the launch would run on the lock-step kernel (fewer than two units per CU), and on a width-192 or width-256 plan.         */
/* Alignment: x16, scratch8 and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: scratch8 and out may overlap neither x16 nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_mlp_fused_planned(ivit_handle h, ivit_mlp_plan p, const int16_t *x16, float scale, const float *bias_int,
                                     const float *sc, const ivit_dyadic *ln_dy, int8_t *scratch8, const int8_t *gelu_table,
                                     ivit_dyadic dy_main, ivit_dyadic dy_res, int16_t *out, int64_t M);
/* The same block tail — norm2 + qact3, Mlp.forward and the residual QuantAct (vit_quant.py:139-142 around layers_quant.py:144-153) — in
 * ONE launch of the LOCK-STEP kernel, at widths 192 and 384 and every token count: a workgroup computes the LayerNorm of a unit's rows
 * (x16 [M, C], the block's 16-bit stream, which is also the identity branch; scale / bias_int / sc / ln_dy as for
 * ivit_layernorm_requant) straight into the unit's activation tile in LDS, one unit ahead of the GEMMs, so norm2's 8-bit rows never
 * exist in memory and there is no scratch argument.  out == ivit_layernorm_requant followed by ivit_mlp_fused_planned.  Always the
 * lock-step kernel, whatever ivit_mlp_plan_select says; grids and unit schedules are those of ivit_mlp_fused_planned on that kernel
 * (ivit_set_cu_share included).  out overlapping x16 is IVIT_ERR_INVALID.  IVIT_ERR_UNSUPPORTED (nothing launched) on a plan of
 * another width (256) and for residual multipliers outside the fast range.                                                       */
/* Alignment: x16 and out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x16 (see above): IVIT_ERR_INVALID, nothing launched. */
int ivit_layernorm_mlp_lockstep_planned(ivit_handle h, ivit_mlp_plan p, const int16_t *x16, float scale, const float *bias_int,
                                        const float *sc, const ivit_dyadic *ln_dy, const int8_t *gelu_table, ivit_dyadic dy_main,
                                        ivit_dyadic dy_res, int16_t *out, int64_t M);
/* PatchMerging's 2x2 gather (swin_quant.py:336-342): x [B,R,R,C] (in_bits 8 or 16) ->
 * int16 [B, (R/2)^2, 4C], channel blocks in the reference's torch.cat order.                  */
/* Alignment: x 16-byte aligned (8-byte at in_bits = 8), out 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_patch_merge_gather(ivit_handle h, const void *x, int in_bits, int B, int R, int C, int16_t *out);
/* The same gather folded into the I-LayerNorm + QuantAct(8) that follows it in PatchMerging.forward (swin_quant.py:336-349:
 * gather, self.norm over 4C, qact1) — x int16 [B,R,R,C] -> out8 int8 [B (R/2)^2, 4C]; the gathered tensor never exists.  Same
 * integers as ivit_patch_merge_gather + ivit_layernorm_requant.  C in {96, 128, 192, 256, 384}; else IVIT_ERR_UNSUPPORTED.      */
/* Alignment: x and out8 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out8 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_patch_merge_layernorm_requant(ivit_handle h, const int16_t *x, int B, int R, int C, float scale,
                                       const float *bias_int, const float *sc, const ivit_dyadic *dy_ch, int8_t *out8);
/* Overlap: out may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_widen_i8_i16(ivit_handle h, const int8_t *x, int16_t *out, int64_t n);
/* PatchMerging's reduction -> qact2 (swin_quant.py:343-349: QuantLinear(4C, 2C, bias = False) then an 8-bit QuantAct) whose consumer is the
 * next stage's 16-bit stream: out16 = clamp8(rq(acc + bias, dy_ch[n])) stored as int16 [M][N] — ivit_linear_i8_requant(bits = 8) followed by
 * ivit_widen_i8_i16 in one launch, same integers.  gemm_glds_kernel's shapes only (K % 32 == 0, K >= 64, not the short-K streaming kernel's):
 * IVIT_ERR_UNSUPPORTED otherwise, nothing launched.                                                                                  */
/* Alignment: x and out16 16-byte aligned; IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: out16 may not overlap x: IVIT_ERR_INVALID, nothing launched. */
int ivit_linear_i8_requant8_store16(ivit_handle h, const int8_t *x, const int8_t *w, const int32_t *bias, const ivit_dyadic *dy_ch,
                                    int16_t *out16, int M, int N, int K);

/* ---- a13  predictions: what validate() does with the model's output (quant_train.py:314-351: output = model(data) at :334, then
 * accuracy(output, target, topk=(1, 5)) at :338, i.e. a top-k of every output row compared with the label), on the device.
 * The output is the head's accumulators times the per-class head scale (quant_modules.py:96-97: F.linear(x_int, weight_integer,
 * bias_integer) * bias_scaling_factor, returned unchanged by vit_quant.py:278-282 / swin_quant.py:560-564):
 *   v[b, c] = fl32(fl32(logits[b, c]) * scale[c])      (int -> fp32 conversion RNE, one multiply, nothing contracted)
 * logits int32 [batch, num_classes], scale float [num_classes] -> idx int32 [batch, k], val float [batch, k] (val may be NULL:
 * indices only).  The ORDER is part of the contract, which torch.topk's is not: descending by value, -0.0 and +0.0 equal, equal values
 * by ascending class index — row b of idx is the first k entries of np.lexsort((arange(num_classes), -(v[b] + 0.0))); val holds the
 * bits of v, -0.0 included.  Non-finite scale entries are OUTSIDE the contract (no frozen model has one).
 * 1 <= k <= min(16, num_classes), IVIT_ERR_INVALID otherwise (nothing launched).  One launch (csrc/ivit_topk.h).                    */
/* Overlap: idx and val may overlap neither logits nor each other: IVIT_ERR_INVALID, nothing launched. */
int ivit_logits_topk(ivit_handle h, const int32_t *logits, const float *scale, int batch, int num_classes, int k, int32_t *idx,
                     float *val);
/* validate()'s `output = model(images)` + `output.topk(...)` (quant_train.py:334, :338) as one call: ivit_vit_forward /
 * ivit_swin_forward of the same arguments (logits is written, with the same integers), then ivit_logits_topk of those logits with
 * `head_scale` (float [num_classes], device: the model's bias_scaling_factor of the head, "head.scale" of the constants blob) on the
 * handle's stream, behind the slices' join.  k is checked before anything is launched.  The *_graph_create forms capture both
 * (replay: ivit_graph_launch).                                                                                                      */
int ivit_vit_predict(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                     const float *head_scale, int k, int32_t *idx, float *val);
int ivit_swin_predict(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                      const float *head_scale, int k, int32_t *idx, float *val);
int ivit_vit_predict_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                  int32_t *logits, const float *head_scale, int k, int32_t *idx, float *val, ivit_graph *out);
int ivit_swin_predict_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes,
                                   int32_t *logits, const float *head_scale, int k, int32_t *idx, float *val, ivit_graph *out);

/* ---- diagnostics (used by the parity tests only) ------------------------------------
 * q_ieee = n / d (compiler's correctly-rounded division) and q_lean = the hoisted-reciprocal
 * FMA sequence the kernels use for constant divisors; must agree bit for bit.            */
int ivit_debug_div(ivit_handle h, const float *n, const float *d, float *q_ieee, float *q_lean,
                   int64_t count);
/* r_ieee = fl(fl(q*d)/d) with the compiler's division and r_markstein = the three-operation form the
 * I-LayerNorm kernel uses (product, exact residual, one correction with RN(1/d)); must agree bit
 * for bit (quant_modules.py:359 x / scaling_factor after :204-206 x * scaling_factor).       */
int ivit_debug_requotient(ivit_handle h, const float *q, const float *d, float *r_ieee, float *r_markstein,
                          int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_H */
