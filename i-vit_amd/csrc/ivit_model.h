// ivit_model.h — native runners for the frozen integer DeiT/ViT and Swin forwards (include/ivit.h,
// "whole-model runner").  Each chains the C-ABI entry points of ivit_hip.hip in the order of the
// reference's forward (vit_quant.py:254-282, swin_quant.py) and owns its ShiftGELU tables and plans.
// What is not about a model is written once, first: SliceRunner (the slice streams, events and handles), fork_join, graph_capture,
// RUN / fused_or, the argument checks several entries share (extents_disjoint, index_list_ok), RunOut (every destination a forward
// can write for its caller, and where a slice ends) and gelu_table.  Then each model: its struct, slice layout, slice body (run_slice,
// overloaded) and create / destroy / queries.  Last, once for both models, the runner entries: slice_view and run_slices (where a
// slice lies in the caller's arrays; what a runner checks, and in which order, before it launches) and one body per kind of entry.
// Included at the end of ivit_hip.hip.
#pragma once
#include <vector>

struct ivit_graph_s {
    ivit_handle h;
    hipGraph_t graph;
    hipGraphExec_t exec;
};

namespace {

// the internal streams of a runner: one stream, "done" event and handle per slice, and the event the slices fork from
struct SliceRunner {
    std::vector<ivit_handle> slice_h;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> done;
    hipEvent_t fork = nullptr;

    // nothing for one slice.  Each resource is owned by the struct as soon as it exists, so destroy() after a failure releases it
    bool create(ivit_handle h, int max_slices) {
        if (max_slices <= 1) return true;
        bool ok = hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < max_slices; ++i) {
            hipStream_t st = nullptr;
            hipEvent_t ev = nullptr;
            ivit_handle sh = nullptr;
            ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
            if (ok) streams.push_back(st);
            ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
            if (ok) done.push_back(ev);
            ok = ok && ivit_create(&sh, h->device, st) == IVIT_OK;
            if (ok) slice_h.push_back(sh);
        }
        return ok;
    }
    void destroy() {
        for (auto sh : slice_h) ivit_destroy(sh);
        for (auto ev : done) (void)hipEventDestroy(ev);
        for (auto st : streams) (void)hipStreamDestroy(st);
        if (fork) (void)hipEventDestroy(fork);
    }
};

inline int slice_begin(int batch, int nslices, int i) { return (int)(((long long)batch * i) / nslices); }
inline int max_slice(int batch, int nslices) { return (batch + nslices - 1) / nslices; }

// body(handle, slice index, first image, images) for each of `nslices` slices of `batch` images: on the caller's handle for one slice,
// else on the internal streams, forked from and joined back into the caller's stream.  A failing slice's error text goes to `h`
template <class Body>
int fork_join(const SliceRunner &r, ivit_handle h, int batch, int nslices, Body &&body) {
    if (nslices == 1) return body(h, 0, 0, batch);
    if (hipEventRecord(r.fork, h->stream) != hipSuccess) return IVIT_ERR_HIP;
    for (int i = 0; i < nslices; ++i) {
        const int b0 = slice_begin(batch, nslices, i), b1 = slice_begin(batch, nslices, i + 1);
        if (hipStreamWaitEvent(r.streams[i], r.fork, 0) != hipSuccess) return IVIT_ERR_HIP;
        r.slice_h[i]->cu_share = std::max(1, persistent_cus(h) / nslices);      // a share of the caller's own share
        const int rc = body(r.slice_h[i], i, b0, b1 - b0);
        if (rc != IVIT_OK) { snprintf(h->err, sizeof(h->err), "%s", r.slice_h[i]->err); return rc; }
        if (hipEventRecord(r.done[i], r.streams[i]) != hipSuccess) return IVIT_ERR_HIP;
    }
    for (int i = 0; i < nslices; ++i)
        if (hipStreamWaitEvent(h->stream, r.done[i], 0) != hipSuccess) return IVIT_ERR_HIP;
    return IVIT_OK;
}

// the *_graph_create forms: `entry(m, args...)`, the eager entry itself (so a refusal names it), captured on the stream of the model's
// handle into an executable graph
template <class M, class Entry, class... Args>
int graph_capture(M *m, ivit_graph *out, Entry entry, Args... args) {
    if (!m) return IVIT_ERR_INVALID;
    ivit_handle h = m->h;
    REQUIRE(h, out, "null argument");
    REQUIRE(h, h->stream != nullptr, "graph capture needs a non-default stream on the handle");
    hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "begin capture: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    const int rc = entry(m, args...);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(h->stream, &graph);
    if (rc != IVIT_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || !graph) { snprintf(h->err, sizeof(h->err), "end capture: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(graph); snprintf(h->err, sizeof(h->err), "instantiate: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    ivit_graph_s *g = new (std::nothrow) ivit_graph_s();
    if (!g) { (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph); return IVIT_ERR_HIP; }
    g->h = h; g->graph = graph; g->exec = exec;
    *out = g;
    return IVIT_OK;
}

// the slice bodies: a failing call ends the slice with its status
#define RUN(call) do { const int rc_ = (call); if (rc_ != IVIT_OK) return rc_; } while (0)
// REQUIRE for a check shared by several entries: the refusal names the entry the caller used
#define REQUIRE_FN(h, fn, cond, msg) do { if (!(cond)) { snprintf((h)->err, sizeof((h)->err), "%s: %s", fn, msg); return IVIT_ERR_INVALID; } } while (0)
// the overlap table of an entry (include/ivit.h, overlapping arguments): every array it reads or writes, as the header spells it.
// extents_disjoint judges the pairs (i, j) with j >= `from`, the first array this caller is responsible for: an entry judges the pairs
// that involve its extra arrays before it calls run_slices, which judges those among images, workspace and logits.  Two arrays that
// are only read may overlap; the first overlap found is the refusal
struct Extent { const void *p; size_t bytes; const char *name; bool read_only; };
template <int N>
int extents_disjoint(ivit_handle h, const char *fn, const Extent (&a)[N], int from) {
    for (int i = 0; i < N; ++i)
        for (int j = std::max(i + 1, from); j < N; ++j)
            if (!(a[i].read_only && a[j].read_only) &&
                !ranges_disjoint(h, fn, a[i].p, a[i].bytes, a[i].name, a[j].p, a[j].bytes, a[j].name, a[i].read_only || a[j].read_only ? OVL_IN : OVL_OUT))
                return IVIT_ERR_INVALID;
    return IVIT_OK;
}
// a caller's list of blocks or stages: `n` strictly ascending indices in [0, sites); `name`: the list as the header spells it
inline int index_list_ok(ivit_handle h, const char *fn, const int *list, int n, const char *name, int sites) {
    bool ok = list && n >= 1 && n <= sites;
    for (int j = 0; ok && j < n; ++j) ok = list[j] >= 0 && list[j] < sites && (j == 0 || list[j] > list[j - 1]);
    if (ok) return IVIT_OK;
    snprintf(h->err, sizeof(h->err), "%s: %s must be 1 .. %d strictly ascending indices in [0, %d)", fn, name, sites, sites);
    return IVIT_ERR_INVALID;
}
// a fused entry point where it takes the case (`fused`: its status, or IVIT_ERR_UNSUPPORTED without calling it), else the launches it
// stands for; any other status of the fused entry is the slice's
template <class Fallback>
int fused_or(int fused, Fallback &&fallback) { return fused == IVIT_ERR_UNSUPPORTED ? fallback() : fused; }

// What a forward writes for its caller: every destination a runner entry can ask for — the whole batch's as the entry fills it in,
// one slice's as run_slice sees it (slice_view).  An absent destination is null or empty; an entry sets only what its model has
struct RunOut {
    explicit RunOut(int32_t *logits_) : logits(logits_) {}
    int32_t *logits;              // the head's accumulators [batch, num_classes]; null: no head launch
    // the features [batch, num_features] (include/ivit_features.h): the final norm (ViT) or the pool (Swin) writes here, not the workspace
    int8_t *feat8 = nullptr;
    // a Swin's final-stage tokens [batch, L, C] (include/ivit_classmap.h), tok_image = L * C: the final norm writes here, the pool reads it
    int8_t *tok8 = nullptr; size_t tok_image = 0;
    // a ViT's class-token probabilities (include/ivit_attnmap.h) of blocks[n], strictly ascending, into attn16 [n, batch, H, T]: one
    // ivit_attention_cls_probs directly behind the block's qkv launch (q and k have the same [B*H, T, dh] layout whichever qkv or
    // attention form the block takes).  image = H * T and plane = batch * H * T elements; a slice's attn16 is its first row of plane 0
    struct {
        const int *blocks = nullptr; int n = 0;
        uint16_t *attn16 = nullptr;
        size_t image = 0, plane = 0;
        uint16_t *rows(int t) const { return attn16 + plane * (size_t)t; }
    } attn;
    // the 16-bit outputs of idx[n], strictly ascending — blocks of a ViT (qact4, vit_quant.py:141-143), stages of a Swin (the stage's
    // last block, in front of PatchMerging) — into the caller's packed hid16 (include/ivit_hidden.h).  Plane j starts start[j] elements
    // in and takes image[j] = T_j * C_j elements per image; a slice's rows follow those of the b0 images before it.  The last launch of
    // a tapped block writes there instead of into the workspace, and from then on the stream `x` is the caller's plane.  The stream is
    // never written in place: every later write goes to a workspace buffer
    struct {
        const int *idx = nullptr; int n = 0;
        int16_t *hid16 = nullptr;
        const size_t *start = nullptr, *image = nullptr; size_t b0 = 0;
        int16_t *rows(int j) const { return hid16 + start[j] + b0 * image[j]; }
    } hid;
    bool any() const { return logits || feat8 || tok8 || attn.n || hid.n; }

    // THE rule for "nothing the caller asked for lies behind this point, the slice ends here": asked behind an attention tap, behind a
    // tapped block or stage and behind a Swin's final norm, with the taps taken so far and whether the final norm has run.  feat8 and
    // logits lie behind everything, a Swin's tok8 behind its last stage.  What the entries ask for — logits, feat8, tok8, the attention
    // tap, the hidden tap; a ViT has no tok8, a Swin no attention tap — the last launch of the slice, and who asks:
    //   logits, alone or with any    the head                                              every entry
    //   feat8, no logits             the final norm (ViT) / the pool (Swin)                features
    //   ViT attn, no logits          the last tapped block's cls_probs                     ivit_vit_attention
    //   ViT hid, no logits           the last tapped block's Mlp launch                    hidden_states
    //   ViT attn and hid             no entry asks for both.  Without logits: the later of the two last taps (the three hand-written
    //                                conditions this rule replaced ran on to the final norm where that was the attention tap)
    //   Swin tok8, no logits         the final norm                                        ivit_swin_class_map, IVIT_CLASSMAP_GIVEN
    //   Swin hid, no logits          the last tapped stage's last Mlp launch, in front of its merge      hidden_states
    bool done(int tapped, int hidden, bool normed) const {
        return !logits && !feat8 && tapped >= attn.n && hidden >= hid.n && (normed || !tok8);
    }
};

// block i's ShiftGELU table
template <class Model>
int8_t *gelu_table(const Model *m, int i) { return m->gelu_tab + (size_t)i * 65536; }

}  // namespace

struct ivit_vit_s {
    // the entries a refusal of the shared workspace query and of the shared forward names
    static constexpr const char *WS_ENTRY = "ivit_vit_workspace_bytes", *FWD_ENTRY = "ivit_vit_forward";
    ivit_handle h;                    // the caller's handle (its stream is the parent stream)
    ivit_vit_config cfg;
    ivit_vit_params prm;
    std::vector<ivit_vit_block> blocks;
    int T, ld, Kp, num_patches;
    bool fused_attention;
    int8_t *gelu_tab;                 // [depth][65536]
    float *rowtab;                    // [depth][256][64] Shiftmax row tables (ivit_shiftmax_rowtable) or null
    std::vector<char> has_rowtab;     // per block: its scale's table lines fit 64 entries and the multipliers are in the fast range
    std::vector<ivit_linear_plan> plans;   // per block: qkv, proj, fc1, fc2 (frozen QuantLinear plans, ivit_linear_plan_create)
    std::vector<ivit_mlp_plan> mlp_plans;  // per block: fused Mlp plan (D = 384 or 192), or null -> fc1 / ShiftGELU / fc2 launches
    int max_slices;
    SliceRunner run;
};

namespace {

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

// byte offsets of the per-slice buffers for `B` images
struct SliceLayout {
    size_t patches, patch16, xa, xb, a8, q, k, vt, ctx8, h8, g8, cls8, s8, p16, total;
};

SliceLayout slice_layout(const ivit_vit_s *m, int B) {
    const ivit_vit_config &c = m->cfg;
    const size_t M = (size_t)B * m->T, D = c.embed_dim, H = c.num_heads, dh = D / H, Hd = c.hidden_dim;
    SliceLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = al256(o + bytes); return at; };
    L.patches = take((size_t)B * m->num_patches * m->Kp);
    L.patch16 = take((size_t)B * m->num_patches * D * 2);
    L.xa = take(M * D * 2);
    L.xb = take(M * D * 2);
    L.a8 = take(M * D);
    L.q = take((size_t)B * H * m->T * dh);
    L.k = take((size_t)B * H * m->T * dh);
    L.vt = take((size_t)B * H * dh * m->ld);
    L.ctx8 = take(M * D);
    L.h8 = take(M * Hd);
    L.g8 = take(M * Hd);
    L.cls8 = take((size_t)B * D);
    L.s8 = L.p16 = 0;
    if (!m->fused_attention) {
        L.s8 = take((size_t)B * H * m->T * m->ld);
        L.p16 = take((size_t)B * H * m->T * m->ld * 2);
    }
    L.total = o;
    return L;
}

// the shapes ivit_mlp_plan_create has a kernel for: width C, hidden size Hd
inline bool mlp_plan_shape(int C, int Hd) {
    return (C == Mlp384Geo::C && Hd == Mlp384Geo::HD) || (C == Mlp256Geo::C && Hd == Mlp256Geo::HD) || (C == Mlp192Geo::C && Hd == Mlp192Geo::HD);
}

// THE rule for "this block's Mlp is one ivit_mlp_fused_planned launch at M tokens": both run_slice bodies and the
// ivit_*_fused_mlp_blocks queries all ask here.  No token-count threshold: at width 192 the fused launch measured faster than
// the three-launch chain at every size tried, 197 tokens (DeiT-T batch 1: 15.8 against 20.0 us) to 200 704 (profiles/README.md)
inline bool mlp_plan_fuses(ivit_mlp_plan mp, ivit_dyadic res_main, ivit_dyadic res_res, long long /*M*/) {
    return mp && rq_fast2(res_main, res_res);
}

// THE rule for "this block's norm1 + qkv is one ivit_layernorm_linear_i8_qkv_ldv_planned launch at B images": run_slice and
// ivit_vit_fused_qkv_blocks ask here.  It is the entry's own acceptance test — a prepared plan (D = 192 or 384, dh = 64) and, for a
// layer that keeps v^T (no Shiftmax row table), width 192.  No token-count threshold: see profiles/README.md, "Width 192 on the
// weights-in-registers GEMM"
inline bool qkv_plan_fuses(const ivit_vit_s *m, int i, int B) {
    const int H = m->cfg.num_heads, ldv = (m->fused_attention && m->has_rowtab[i]) ? 0 : m->ld;
    return qkv_ws_ok(m->plans[4 * i], B, m->T, H, m->cfg.embed_dim / H, ldv);
}

// THE rule for "the last block runs its attention, proj, norm2 and Mlp on the class-token rows only": run_slice and ivit_vit_cls_tail
// ask here.  Everything behind a block's attention is row-local and a context row depends on its own q row alone, while the head reads
// row 0 of each image only — so behind the last block's qkv GEMM (k and v need every token) the other T - 1 rows are work nobody
// reads.  Needs the fused attention (its class-token form) and the dead PatchEmbed buffers large enough for the compact rows
inline bool cls_tail(const ivit_vit_s *m) {
    return m->fused_attention && (size_t)m->num_patches * m->Kp >= (size_t)m->cfg.embed_dim;
}

// block i's attention on the fused kernel, in the Shiftmax form the block has tables for (v row-major, ldv = 0, with a row table; v^T
// otherwise).  cls: the class-token form — the context of
// token 0 of every image into `ctx` [B, D], its identity row of x16 into x_cls
int vit_attention(const ivit_vit_s *m, ivit_handle h, int i, const int8_t *q, const int8_t *k, const int8_t *vt, int8_t *ctx, int B, int ldv,
                  bool cls, const int16_t *x16, int16_t *x_cls) {
    const ivit_vit_block &b = m->blocks[i];
    const int T = m->T, H = m->cfg.num_heads, dh = m->cfg.embed_dim / H;
    if (m->has_rowtab[i]) {      // one gather per score (round 6)
        const float *rowtab = m->rowtab + (size_t)i * 256 * 64;
        return cls ? ivit_attention_fused_rowlut_cls(h, q, k, vt, b.dy_qk, b.s_softmax, rowtab, b.exp_dmin, b.dy_pv, ctx, x16, x_cls, B, H, T, dh, ldv)
                   : ivit_attention_fused_rowlut(h, q, k, vt, b.dy_qk, b.s_softmax, rowtab, b.exp_dmin, b.dy_pv, ctx, B, H, T, dh, ldv);
    }
    if (b.exp_aq)
        return cls ? ivit_attention_fused_lut_cls(h, q, k, vt, b.dy_qk, b.s_softmax, b.exp_aq, b.exp_t, b.exp_cls, b.exp_nc, b.exp_tcount, b.exp_dmin,
                                                  b.dy_pv, ctx, x16, x_cls, B, H, T, dh, ldv)
                   : ivit_attention_fused_lut(h, q, k, vt, b.dy_qk, b.s_softmax, b.exp_aq, b.exp_t, b.exp_cls, b.exp_nc, b.exp_tcount, b.exp_dmin,
                                              b.dy_pv, ctx, B, H, T, dh, ldv);
    return cls ? ivit_attention_fused_cls(h, q, k, vt, b.dy_qk, b.s_softmax, b.dy_pv, ctx, x16, x_cls, B, H, T, dh, ldv)
               : ivit_attention_fused(h, q, k, vt, b.dy_qk, b.s_softmax, b.dy_pv, ctx, B, H, T, dh, ldv);
}

// one slice of `B` images on handle `h`, into the slice's view `out` of what the caller asked for (RunOut: what each destination is,
// and done(), where the slice ends)
// `Blay`: the images the slice's buffers are laid out for (layout_images)
// With a hidden tap the proj launch writes the workspace buffer `x` is not (other), the Mlp launch the one its input is not — or the
// caller's plane.  A tapped last block runs on all rows (the class-token tail has B of them)
int run_slice(const ivit_vit_s *m, ivit_handle h, const int8_t *images, int B, int Blay, char *ws, const RunOut &out) {
    const ivit_vit_config &c = m->cfg;
    const ivit_vit_params &P = m->prm;
    const int T = m->T, D = c.embed_dim, H = c.num_heads, dh = D / H, Hd = c.hidden_dim, ld = m->ld;
    const int M = B * T;
    const SliceLayout L = slice_layout(m, Blay);
    int8_t *patches = (int8_t *)(ws + L.patches), *a8 = (int8_t *)(ws + L.a8), *q = (int8_t *)(ws + L.q),
           *k = (int8_t *)(ws + L.k), *vt = (int8_t *)(ws + L.vt), *ctx8 = (int8_t *)(ws + L.ctx8),
           *h8 = (int8_t *)(ws + L.h8), *g8 = (int8_t *)(ws + L.g8), *cls8 = out.feat8 ? out.feat8 : (int8_t *)(ws + L.cls8);
    int16_t *patch16 = (int16_t *)(ws + L.patch16), *const xa = (int16_t *)(ws + L.xa), *const xb = (int16_t *)(ws + L.xb), *x = xa;
    // the workspace stream buffer that `cur` is not (xa behind a caller's plane): without a tap xa -> xb -> xa, block after block
    auto other = [&](const int16_t *cur) { return cur == xa ? xb : xa; };
    // the class-token tail computes B rows of the last block: not where the caller asked for that block's output
    const bool tailed = cls_tail(m) && !(out.hid.n && out.hid.idx[out.hid.n - 1] == c.depth - 1);
    // PatchEmbed + class token + position embedding: one GEMM launch that gathers its A rows from the images and finishes the rows in its
    // epilogue (round 6), or im2col -> GEMM -> embed_finish where that form does not apply
    RUN(fused_or((m->Kp == c.in_chans * c.patch_size * c.patch_size)
                     ? ivit_patch_embed(h, images, B, c.in_chans, c.img_size, c.img_size, c.patch_size, P.pe_w, P.pe_b, P.pe_dy, P.z_cls, P.pos, P.dy_x, P.dy_pos, x, D)
                     : IVIT_ERR_UNSUPPORTED,
                 [&] {
                     RUN(ivit_im2col_patch(h, images, B, c.in_chans, c.img_size, c.img_size, c.patch_size, patches));
                     RUN(ivit_linear_i8_requant(h, patches, P.pe_w, P.pe_b, P.pe_dy, 16, patch16, B * m->num_patches, D, m->Kp));
                     return ivit_embed_finish(h, patch16, P.z_cls, P.pos, P.dy_x, P.dy_pos, x, B, T, D);
                 }));
    int tapped = 0, hidden = 0;
    for (int i = 0; i < c.depth; ++i) {
        const ivit_vit_block &b = m->blocks[i];
        // a layer on the row-table attention takes v ROW-major (ldv = 0: the qkv GEMM stores 16 bytes per lane instead of 16 byte
        // stores, the attention kernel transposes on its way into the LDS); the other attention forms read v^T
        const int ldv = (m->fused_attention && m->has_rowtab[i]) ? 0 : ld;
        // last block: from the attention on, the B class-token rows only (cls_tail), compact in the buffers PatchEmbed has left:
        // context rows in `patches`, the identity rows — copied by the attention launch — in `patch16`
        const bool tail = i == c.depth - 1 && tailed;
        const int Mb = tail ? B : M;      // rows behind the attention
        // norm1's 8-bit output has one consumer: where the qkv GEMM keeps a CU's tokens in LDS it is computed there (round 6; D = 192 too,
        // with v in either layout)
        RUN(fused_or(qkv_plan_fuses(m, i, B) ? ivit_layernorm_linear_i8_qkv_ldv_planned(h, m->plans[4 * i], x, b.s_ln1, b.n1_bias_int, b.n1_sc, b.n1_dy,
                                                                                        q, k, vt, B, T, H, dh, ldv)
                                             : IVIT_ERR_UNSUPPORTED,
                     [&] {
                         RUN(ivit_layernorm_requant(h, x, M, D, D, b.s_ln1, b.n1_bias_int, b.n1_sc, b.n1_dy, a8));
                         return ivit_linear_i8_qkv_planned(h, m->plans[4 * i], a8, q, k, vt, B, T, H, dh, ldv);
                     }));
        if (tapped < out.attn.n && out.attn.blocks[tapped] == i) {
            RUN(ivit_attention_cls_probs(h, q, k, b.dy_qk, b.s_softmax, out.attn.rows(tapped), B, H, T, dh));
            if (out.done(++tapped, hidden, false)) return IVIT_OK;
        }
        int16_t *y = other(x);          // proj's destination
        if (tail) {
            ctx8 = patches;
            RUN(vit_attention(m, h, i, q, k, vt, ctx8, B, ldv, true, x, patch16));
            x = patch16;                // [B, D]; proj writes y, the Mlp writes patch16 again
        } else if (m->fused_attention) {
            RUN(vit_attention(m, h, i, q, k, vt, ctx8, B, ldv, false, nullptr, nullptr));
        } else {
            int8_t *s8 = (int8_t *)(ws + L.s8);
            uint16_t *p16 = (uint16_t *)(ws + L.p16);
            RUN(ivit_attn_qk_requant(h, q, k, b.dy_qk, s8, B * H, T, dh, ld));
            RUN(ivit_shiftmax(h, s8, (int64_t)B * H * T, T, ld, b.s_softmax, 16, p16, ld));
            RUN(ivit_attn_pv_requant(h, p16, vt, b.dy_pv, ctx8, B, H, T, dh, ld, ld));
        }
        // attn.proj + qact2 with the identity branch, then norm2 + qact3 and the Mlp.  norm2 rides in the HEAD of the fused Mlp's launch
        // (ivit_layernorm_mlp_fused_planned) where the role-split kernel takes the shape, else in the activation tiles of the lock-step
        // kernel (ivit_layernorm_mlp_lockstep_planned: D = 192, D = 384 below two units per CU, the class-token tail) where
        // ln_mlp_plan_fuses says so; in the tail of the proj launch it measured slower (profiles/README.md)
        const bool mlp_fast = mlp_plan_fuses(m->mlp_plans[i], b.res2_main, b.res2_res, Mb);
        const bool ln_lockstep = ln_mlp_plan_fuses(h, m->mlp_plans[i], b.res2_main, b.res2_res, Mb) == LN_MLP_LOCKSTEP;
        RUN(ivit_linear_i8_requant_residual_planned(h, m->plans[4 * i + 1], ctx8, b.res1_main, b.res1_res, x, y, Mb));
        const bool hid_here = hidden < out.hid.n && out.hid.idx[hidden] == i;
        // the Mlp's destination: the caller's plane for a tapped block, else the workspace buffer its input is not (the tail: patch16,
        // which the proj launch has read)
        { int16_t *t = x; x = y; y = hid_here ? out.hid.rows(hidden) : tail ? t : other(x); }
        const int8_t *tab = gelu_table(m, i);
        RUN(fused_or(mlp_fast ? ivit_layernorm_mlp_fused_planned(h, m->mlp_plans[i], x, b.s_ln2, b.n2_bias_int, b.n2_sc, b.n2_dy, a8, tab, b.res2_main,
                                                                 b.res2_res, y, Mb)
                              : IVIT_ERR_UNSUPPORTED,
                     [&] {
                         return fused_or(ln_lockstep ? ivit_layernorm_mlp_lockstep_planned(h, m->mlp_plans[i], x, b.s_ln2, b.n2_bias_int, b.n2_sc,
                                                                                           b.n2_dy, tab, b.res2_main, b.res2_res, y, Mb)
                                                     : IVIT_ERR_UNSUPPORTED,
                                         [&] {
                                             RUN(ivit_layernorm_requant(h, x, Mb, D, D, b.s_ln2, b.n2_bias_int, b.n2_sc, b.n2_dy, a8));
                                             if (mlp_fast)       // hidden tensor stays in LDS
                                                 return ivit_mlp_fused_planned(h, m->mlp_plans[i], a8, tab, b.res2_main, b.res2_res, x, y, Mb);
                                             RUN(ivit_linear_i8_requant_planned(h, m->plans[4 * i + 2], a8, 8, h8, Mb));
                                             RUN(ivit_shiftgelu_requant_lut(h, h8, Mb, Hd, tab, g8));
                                             return ivit_linear_i8_requant_residual_planned(h, m->plans[4 * i + 3], g8, b.res2_main, b.res2_res, x, y, Mb);
                                         });
                     }));
        x = y;
        if (hid_here && out.done(tapped, ++hidden, false)) return IVIT_OK;
    }
    // final norm on the class-token rows only (row stride T*D; D where the last block left them compact), then the head's int32
    // accumulators
    RUN(ivit_layernorm_requant(h, x, B, D, tailed ? (int64_t)D : (int64_t)T * D, P.s_ln, P.n_bias_int, P.n_sc, P.n_dy, cls8));
    if (out.logits) RUN(ivit_linear_i8(h, cls8, P.head_w, P.head_b, out.logits, B, c.num_classes, D));
    return IVIT_OK;
}

// what run_slices asks of a model: the workspace bytes of one slice of `Bmax` images, the images a slice of `nb` lays its buffers
// out for — those of the LARGEST slice of the forward, so the regions zeroed by ivit_vit_workspace_init are the ones the kernels see
// whatever the (ragged) slice sizes are —, the width of a features row, and run_slice
inline size_t slice_stride(const ivit_vit_s *m, int Bmax) { return slice_layout(m, Bmax).total; }
inline int layout_images(const ivit_vit_s *, int, int Bmax) { return Bmax; }
inline int num_features(const ivit_vit_s *m) { return m->cfg.embed_dim; }
// THE rule for "a slice of this many images is more than the model's launches take" (run_slices refuses a larger one before anything
// is launched): an image of a slice is one gridDim.y of the embedding launches (ivit_patch_embed, ivit_embed_finish: B <= 65535), and
// without the fused attention every (image, head) is one matrix of the batched products (ivit_attn_qk_requant: B * H <= 65535)
inline int max_slice_images(const ivit_vit_s *m) { return m->fused_attention ? 65535 : 65535 / m->cfg.num_heads; }
// ... and of its hidden states (include/ivit_hidden.h): how many sites it has (blocks), the tokens and the width of site i's plane
inline int hidden_sites(const ivit_vit_s *m) { return m->cfg.depth; }
inline int hidden_tokens(const ivit_vit_s *m, int) { return m->T; }
inline int hidden_width(const ivit_vit_s *m, int) { return m->cfg.embed_dim; }

}  // namespace

extern "C" {

int ivit_vit_create(ivit_handle h, const ivit_vit_config *cfg, const ivit_vit_params *params, int max_slices,
                    ivit_vit *out) {
    CHECK_H(h);
    REQUIRE(h, cfg && params && out && params->blocks_host, "null argument");
    REQUIRE(h, cfg->depth > 0 && cfg->embed_dim > 0 && cfg->num_heads > 0 && cfg->embed_dim % cfg->num_heads == 0 &&
                   cfg->patch_size > 0 && cfg->img_size % cfg->patch_size == 0 && cfg->hidden_dim > 0 &&
                   cfg->num_classes > 0 && cfg->in_chans > 0,
            "bad model configuration");
    REQUIRE(h, max_slices >= 1 && max_slices <= 16, "max_slices must be in [1, 16]");
    ivit_vit_s *m = new (std::nothrow) ivit_vit_s();
    if (!m) return IVIT_ERR_HIP;
    m->h = h;
    m->cfg = *cfg;
    m->prm = *params;
    m->blocks.assign(params->blocks_host, params->blocks_host + cfg->depth);
    m->prm.blocks_host = m->blocks.data();
    const int g = cfg->img_size / cfg->patch_size;
    m->num_patches = g * g;
    m->T = m->num_patches + 1;
    m->ld = (m->T + 15) / 16 * 16;
    m->Kp = cfg->in_chans * cfg->patch_size * cfg->patch_size;
    m->fused_attention = (cfg->embed_dim / cfg->num_heads == 64) && m->T <= 640;
    m->gelu_tab = nullptr;
    m->rowtab = nullptr;
    m->has_rowtab.assign(cfg->depth, 0);
    m->max_slices = max_slices;
    hipError_t e = hipMalloc((void **)&m->gelu_tab, (size_t)cfg->depth * 65536);
    if (e == hipSuccess && m->fused_attention) e = hipMalloc((void **)&m->rowtab, (size_t)cfg->depth * 256 * 64 * sizeof(float));
    if (e != hipSuccess) {
        snprintf(h->err, sizeof(h->err), "ivit_vit_create: hipMalloc: %s", hipGetErrorString(e));
        delete m;
        return IVIT_ERR_HIP;
    }
    for (int i = 0; i < cfg->depth; ++i) {
        int rc = ivit_shiftgelu_build_table(h, m->blocks[i].s_gelu, m->blocks[i].dy_gelu, gelu_table(m, i));
        if (rc != IVIT_OK) { ivit_vit_destroy(m); return rc; }
        // frozen QuantLinear plans: per-channel multipliers and the exactness bounds of the pipelined GEMMs
        const ivit_vit_block &b = m->blocks[i];
        if (m->rowtab && b.exp_aq && 1 - b.exp_dmin <= 64 && attn_fast(b.dy_qk, b.dy_pv)) {
            rc = ivit_shiftmax_rowtable(h, b.exp_aq, b.exp_t, b.exp_cls, b.exp_nc, b.exp_tcount, b.exp_dmin, m->rowtab + (size_t)i * 256 * 64);
            if (rc != IVIT_OK) { ivit_vit_destroy(m); return rc; }
            m->has_rowtab[i] = 1;
        }
        const int D = cfg->embed_dim, Hd = cfg->hidden_dim;
        const struct { const int8_t *w; const int32_t *bias; const ivit_dyadic *dy; int N, K; } lin[4] = {
            {b.qkv_w, b.qkv_b, b.qkv_dy, 3 * D, D}, {b.proj_w, b.proj_b, b.proj_dy, D, D},
            {b.fc1_w, b.fc1_b, b.fc1_dy, Hd, D}, {b.fc2_w, b.fc2_b, b.fc2_dy, D, Hd}};
        for (int k = 0; k < 4; ++k) {
            ivit_linear_plan pl = nullptr;
            rc = ivit_linear_plan_create(h, lin[k].w, lin[k].bias, lin[k].dy, lin[k].N, lin[k].K, &pl);
            if (rc != IVIT_OK) { ivit_vit_destroy(m); return rc; }
            // the qkv layer of a D = 192 or 384, dh = 64 model also runs on gemm_ws_qkv_kernel (weights in its fragment order)
            if (k == 0 && ws_width(D) && D / cfg->num_heads == 64) (void)ivit_linear_plan_prepare_ws(h, pl);
            if (k == 1 && ws_width(D)) (void)ivit_linear_plan_prepare_ws(h, pl);      // attn.proj + residual on the same kernel
            m->plans.push_back(pl);
        }
        ivit_mlp_plan mp = nullptr;
        if (mlp_plan_shape(D, Hd) && ivit_mlp_plan_create(h, m->plans[4 * i + 2], m->plans[4 * i + 3], &mp) != IVIT_OK) mp = nullptr;
        m->mlp_plans.push_back(mp);
    }
    if (!m->run.create(h, max_slices)) {
        snprintf(h->err, sizeof(h->err), "ivit_vit_create: stream/event creation failed");
        ivit_vit_destroy(m);
        return IVIT_ERR_HIP;
    }
    *out = m;
    return IVIT_OK;
}

int ivit_vit_destroy(ivit_vit m) {
    if (!m) return IVIT_ERR_INVALID;
    m->run.destroy();
    if (m->gelu_tab) (void)hipFree(m->gelu_tab);
    if (m->rowtab) (void)hipFree(m->rowtab);
    for (auto mp : m->mlp_plans) if (mp) (void)ivit_mlp_plan_destroy(mp);
    for (auto pl : m->plans) (void)ivit_linear_plan_destroy(pl);
    delete m;
    return IVIT_OK;
}

int ivit_vit_fused_mlp_blocks(ivit_vit m, int batch, int *blocks) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE(m->h, blocks && batch > 0, "bad arguments");
    int n = 0;
    for (int i = 0; i < m->cfg.depth; ++i)
        n += mlp_plan_fuses(m->mlp_plans[i], m->blocks[i].res2_main, m->blocks[i].res2_res, (long long)batch * m->T);
    *blocks = n;
    return IVIT_OK;
}

int ivit_vit_fused_ln_mlp_blocks(ivit_vit m, int batch, int *blocks) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE(m->h, blocks && batch > 0, "bad arguments");
    int n = 0;
    for (int i = 0; i < m->cfg.depth; ++i) {
        const bool tail = i == m->cfg.depth - 1 && cls_tail(m);
        n += ln_mlp_plan_fuses(m->h, m->mlp_plans[i], m->blocks[i].res2_main, m->blocks[i].res2_res, tail ? batch : (long long)batch * m->T) !=
             LN_MLP_TWO_LAUNCHES;
    }
    *blocks = n;
    return IVIT_OK;
}

int ivit_vit_fused_qkv_blocks(ivit_vit m, int batch, int *blocks) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE(m->h, blocks && batch > 0, "bad arguments");
    int n = 0;
    for (int i = 0; i < m->cfg.depth; ++i) n += qkv_plan_fuses(m, i, batch);
    *blocks = n;
    return IVIT_OK;
}

int ivit_vit_cls_tail(ivit_vit m, int batch, int *on) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE(m->h, on && batch > 0, "bad arguments");
    *on = cls_tail(m) ? 1 : 0;
    return IVIT_OK;
}

int ivit_vit_workspace_init(ivit_vit m, void *workspace, size_t bytes, int batch, int nslices) {
    if (!m) return IVIT_ERR_INVALID;
    size_t need = 0;
    int rc = ivit_vit_workspace_bytes(m, batch, nslices, &need);
    if (rc != IVIT_OK) return rc;
    REQUIRE(m->h, workspace && bytes >= need, "workspace too small");
    REQUIRE(m->h, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const SliceLayout L = slice_layout(m, max_slice(batch, nslices));
    for (int i = 0; i < nslices; ++i) {
        char *ws = (char *)workspace + L.total * (size_t)i;
        const size_t vt_bytes = (size_t)max_slice(batch, nslices) * m->cfg.num_heads * (m->cfg.embed_dim / m->cfg.num_heads) * m->ld;
        if (hipMemsetAsync(ws + L.vt, 0, vt_bytes, m->h->stream) != hipSuccess) return IVIT_ERR_HIP;
        if (!m->fused_attention) {
            const size_t pb = (size_t)max_slice(batch, nslices) * m->cfg.num_heads * m->T * m->ld * 2;
            if (hipMemsetAsync(ws + L.p16, 0, pb, m->h->stream) != hipSuccess) return IVIT_ERR_HIP;
        }
    }
    return IVIT_OK;
}

}  // extern "C"

// =====================================================================================================
// Swin runner
struct ivit_swin_s {
    static constexpr const char *WS_ENTRY = "ivit_swin_workspace_bytes", *FWD_ENTRY = "ivit_swin_forward";
    ivit_handle h;
    ivit_swin_config cfg;
    ivit_swin_params prm;
    std::vector<ivit_swin_block> blocks;
    std::vector<ivit_swin_merge> merges;
    int grid, nblocks;
    ivit_dyadic dy_qact1_host;        // host copy of prm.dy_qact1[0]
    bool fused_mlp;                   // stage-0 Mlp in one kernel (ivit_mlp_fused: C = 96 or C = 128)
    std::vector<ivit_linear_plan> mlp_lin;   // per block: fc1, fc2 plans of the C = 384, C = 256 and C = 192 stages (null elsewhere)
    std::vector<ivit_mlp_plan> mlp_plans;    // per block: fused Mlp plan (C = 384 / hidden 1536, C = 256 / hidden 1024, C = 192 / hidden 768) or null
    std::vector<ivit_linear_plan> lin_plans; // per block: qkv, proj plans prepared for gemm_ws_qkv_kernel where C == 384, else null
    int8_t *gelu_tab;                 // [nblocks][65536]
    int max_slices;
    SliceRunner run;
};

namespace {

struct SwinLayout { size_t patches, a8, xa, xb, xc, zf, qkv, ctx, h8, g8, pool, total; };

SwinLayout swin_layout(const ivit_swin_s *m, int B) {
    const ivit_swin_config &c = m->cfg;
    const size_t M0 = (size_t)B * m->grid * m->grid, E = c.embed_dim;
    SwinLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = al256(o + bytes + 64); return at; };
    L.patches = take(M0 * c.in_chans * c.patch_size * c.patch_size);
    L.a8 = take(M0 * E);
    L.xa = take(M0 * E * 2);
    L.xb = take(M0 * E * 2);
    L.xc = take(M0 * E * 2);
    L.zf = take(M0 * E * 4);
    L.qkv = take(M0 * 3 * E);
    L.ctx = take(M0 * E);
    L.h8 = take(M0 * c.mlp_ratio * E);
    L.g8 = take(M0 * c.mlp_ratio * E);
    L.pool = take((size_t)B * (E << (c.num_layers - 1)));
    L.total = o;
    return L;
}

int swin_ln(const ivit_swin_s *m, ivit_handle h, const int16_t *x, long long M, int C, float s_in, const ivit_ln_params &n,
            int L, bool token_order, int8_t *out8) {
    if (token_order) return ivit_layernorm_tokenorder_requant(h, x, M, C, s_in, n.bias_int, n.sc, n.dy, L, out8);
    return ivit_layernorm_requant(h, x, M, C, C, s_in, n.bias_int, n.sc, n.dy, out8);
}

// how block `bi` (width C) issues its Mlp at M tokens: 0 = fc1 / ShiftGELU / fc2, 1 = ivit_mlp_fused (narrow stage), 2 = ivit_mlp_fused_planned
int swin_mlp_mode(const ivit_swin_s *m, int bi, int C, long long M) {
    if (C == 96 && m->cfg.mlp_ratio == 4 && m->fused_mlp) return 1;
    // C = 128 (Swin-B stage 0): the same entry, which at this width takes residual multipliers in the fast range only
    if (C == Mlp128Geo::C && m->cfg.mlp_ratio == 4 && m->fused_mlp && rq_fast2(m->blocks[bi].res2_main, m->blocks[bi].res2_res)) return 1;
    return mlp_plan_fuses(m->mlp_plans[bi], m->blocks[bi].res2_main, m->blocks[bi].res2_res, M) ? 2 : 0;
}

// one slice of `B` images on handle `h`, into the slice's view `out` of what the caller asked for (RunOut), its buffers laid out for
// `Blay` images.  As in the ViT's run_slice the stream is never written in place; behind a tapped stage the merge's reduction writes the
// next stage's stream into the workspace, never into the caller's plane
int run_slice(const ivit_swin_s *m, ivit_handle h, const int8_t *images, int B, int Blay, char *ws, const RunOut &out) {
    const ivit_swin_config &c = m->cfg;
    const ivit_swin_params &P = m->prm;
    const SwinLayout Lw = swin_layout(m, Blay);
    int8_t *patches = (int8_t *)(ws + Lw.patches), *a8 = (int8_t *)(ws + Lw.a8), *qkv = (int8_t *)(ws + Lw.qkv),
           *ctx = (int8_t *)(ws + Lw.ctx), *h8 = (int8_t *)(ws + Lw.h8), *g8 = (int8_t *)(ws + Lw.g8),
           *pool = out.feat8 ? out.feat8 : (int8_t *)(ws + Lw.pool);
    int16_t *const xa = (int16_t *)(ws + Lw.xa), *const xb = (int16_t *)(ws + Lw.xb), *x = xa, *t16 = (int16_t *)(ws + Lw.xc);
    auto other = [&](const int16_t *cur) { return cur == xa ? xb : xa; };      // the workspace stream buffer that `cur` is not
    int hidden = 0;
    float *zf = (float *)(ws + Lw.zf);
    const int E = c.embed_dim;
    int res = m->grid, L = res * res;
    long long M = (long long)B * L;
    const int Kp = c.in_chans * c.patch_size * c.patch_size;
    // PatchEmbed: conv -> qact_before_norm(8) -> norm (token-order sums) -> qact(16) -> qact1(16)
    RUN(ivit_im2col_patch(h, images, B, c.in_chans, c.img_size, c.img_size, c.patch_size, patches));
    RUN(ivit_linear_i8_requant(h, patches, P.pe.w, P.pe.b, P.pe.dy, 8, a8, (int)M, E, Kp));
    RUN(ivit_patch_norm_tokenorder(h, a8, M, E, P.s_bn, P.pn.bias_int, P.pn.sc, P.pn.dy, m->dy_qact1_host, L, x));
    int bi = 0;
    for (int li = 0; li < c.num_layers; ++li) {
        const int C = E << li, heads = c.num_heads[li];
        for (int bj = 0; bj < c.depths[li]; ++bj, ++bi) {
            const ivit_swin_block &b = m->blocks[bi];
            const int shift = (bj % 2 == 0 || res <= c.window_size) ? 0 : c.window_size / 2;
            const int wsz = res <= c.window_size ? res : c.window_size;     // SwinTransformerBlock.__init__
            const ivit_linear_plan *lp = &m->lin_plans[2 * bi];
            int16_t *y = other(x);      // proj's destination
            // norm1 inside the qkv launch where that layer runs on gemm_ws_qkv_kernel (C = 384, activations in natural token order)
            RUN(fused_or((lp[0] && li != 0) ? ivit_layernorm_linear_i8_requant_planned(h, lp[0], x, b.s_in, b.n1.bias_int, b.n1.sc, b.n1.dy, qkv, (int)M)
                                            : IVIT_ERR_UNSUPPORTED,
                         [&] {
                             RUN(swin_ln(m, h, x, M, C, b.s_in, b.n1, L, li == 0, a8));
                             return lp[0] ? ivit_linear_i8_requant_planned(h, lp[0], a8, 8, qkv, (int)M)
                                          : ivit_linear_i8_requant(h, a8, b.qkv.w, b.qkv.b, b.qkv.dy, 8, qkv, (int)M, 3 * C, C);
                         }));
            if (b.exp_aq)
                RUN(ivit_window_attention_fused_lut(h, qkv, b.dy_qk, b.dy_a, b.relb, b.s_softmax, b.exp_aq, b.exp_t, b.exp_cls,
                                                    b.exp_nc, b.exp_tcount, b.exp_dmin, b.dy_pv, ctx, B, res, wsz,
                                                    shift, heads, C / heads));
            else
                RUN(ivit_window_attention_fused(h, qkv, b.dy_qk, b.dy_a, b.relb, b.s_softmax, b.dy_pv, ctx, B, res,
                                                wsz, shift, heads, C / heads));
            if (lp[1]) RUN(ivit_linear_i8_requant_residual_planned(h, lp[1], ctx, b.res1_main, b.res1_res, x, y, (int)M));
            else RUN(ivit_linear_i8_requant_residual(h, ctx, b.proj.w, b.proj.b, b.proj.dy, b.res1_main, b.res1_res, x, y, (int)M, C, C));
            // the Mlp's destination: the caller's plane for the last block of a tapped stage, else the workspace buffer its input is not
            const bool hid_here = hidden < out.hid.n && out.hid.idx[hidden] == li && bj == c.depths[li] - 1;
            x = y;
            y = hid_here ? out.hid.rows(hidden) : other(x);
            const int mlp_mode = swin_mlp_mode(m, bi, C, M);
            // norm2 is a launch of its own in every stage.  (In the head of the C = 384 stage's fused Mlp it measured slower: Swin-T b256,
            // two slices, 4.76 against 4.70 ms same-box; the LayerNorm launch of one slice overlaps the other slice's kernels)
            RUN(swin_ln(m, h, x, M, C, b.s_mid, b.n2, L, li == 0, a8));
            if (mlp_mode == 1) {                                    // narrow stage: hidden tensor stays in LDS
                RUN(ivit_mlp_fused(h, a8, b.fc1.w, b.fc1.b, b.fc1.dy, gelu_table(m, bi), b.fc2.w, b.fc2.b,
                                   b.fc2.dy, b.res2_main, b.res2_res, x, y, M, C, 4 * C));
            } else if (mlp_mode == 2) {                             // C = 192, C = 256 and C = 384 stages: weights streamed, hidden tile in LDS
                RUN(ivit_mlp_fused_planned(h, m->mlp_plans[bi], a8, gelu_table(m, bi), b.res2_main, b.res2_res, x, y, M));
            } else {
                RUN(ivit_linear_i8_requant(h, a8, b.fc1.w, b.fc1.b, b.fc1.dy, 8, h8, (int)M, c.mlp_ratio * C, C));
                RUN(ivit_shiftgelu_requant_lut(h, h8, M, c.mlp_ratio * C, gelu_table(m, bi), g8));
                RUN(ivit_linear_i8_requant_residual(h, g8, b.fc2.w, b.fc2.b, b.fc2.dy, b.res2_main, b.res2_res, x, y, (int)M, C, c.mlp_ratio * C));
            }
            x = y;
            if (hid_here && out.done(0, ++hidden, false)) return IVIT_OK;
        }
        if (li < c.num_layers - 1) {     // PatchMerging: gather -> LN(4C) -> qact1(8) -> reduction -> qact2(8)
            const ivit_swin_merge &g = m->merges[li];
            // the 2 x 2 gather rides in the LayerNorm's loads (round 6: as a pass of its own it was 32 us per merge at Swin-T b256)
            const int res_in = res;
            res /= 2;
            L = res * res;
            M = (long long)B * L;
            RUN(fused_or(ivit_patch_merge_layernorm_requant(h, x, B, res_in, C, g.s_in, g.n.bias_int, g.n.sc, g.n.dy, a8), [&] {
                RUN(ivit_patch_merge_gather(h, x, 16, B, res_in, C, t16));
                return swin_ln(m, h, t16, M, 4 * C, g.s_in, g.n, L, false, a8);
            }));
            if (x != xa && x != xb) x = xa;      // behind a tapped stage `x` is the caller's plane: the next stage's stream starts in the workspace
            // reduction -> qact2(8), stored as the 16-bit stream the next stage reads (round 6: the widening pass was 16 us per merge)
            RUN(fused_or(ivit_linear_i8_requant8_store16(h, a8, g.red.w, nullptr, g.red.dy, x, (int)M, 2 * C, 4 * C), [&] {
                RUN(ivit_linear_i8_requant(h, a8, g.red.w, nullptr, g.red.dy, 8, ctx, (int)M, 2 * C, 4 * C));
                return ivit_widen_i8_i16(h, ctx, x, M * 2 * C);
            }));
        }
    }
    const int C = E << (c.num_layers - 1);
    if (out.tok8) a8 = out.tok8;
    RUN(swin_ln(m, h, x, M, C, P.s_norm_in, P.n, L, false, a8));
    if (out.done(0, hidden, true)) return IVIT_OK;
    RUN((L & 1) ? ivit_avgpool_requant(h, a8, B, L, C, P.dy_pool, pool)
                : ivit_avgpool_requant_scaled(h, a8, B, L, C, P.s_pool, P.dy_pool, pool));
    if (out.logits) RUN(ivit_linear_i8(h, pool, P.head_w, P.head_b, out.logits, B, c.num_classes, C));
    return IVIT_OK;
}

// what run_slices asks of a model, as for the ViT.  A slice lays its buffers out for its own images
inline size_t slice_stride(const ivit_swin_s *m, int Bmax) { return swin_layout(m, Bmax).total; }
inline int layout_images(const ivit_swin_s *, int nb, int) { return nb; }
inline int num_features(const ivit_swin_s *m) { return m->cfg.embed_dim << (m->cfg.num_layers - 1); }
// no launch of a Swin slice has an image per gridDim.y (ivit_im2col_patch takes its one-dimensional grid beyond 65535 images)
inline int max_slice_images(const ivit_swin_s *) { return 0x7fffffff; }
inline int final_tokens(const ivit_swin_s *m) { const int r = m->grid >> (m->cfg.num_layers - 1); return r * r; }
// its hidden states are by stage: (grid >> s)^2 tokens of width embed_dim << s
inline int hidden_sites(const ivit_swin_s *m) { return m->cfg.num_layers; }
inline int hidden_tokens(const ivit_swin_s *m, int s) { const int r = m->grid >> s; return r * r; }
inline int hidden_width(const ivit_swin_s *m, int s) { return m->cfg.embed_dim << s; }

}  // namespace

extern "C" {

int ivit_swin_destroy(ivit_swin m) {
    if (!m) return IVIT_ERR_INVALID;
    m->run.destroy();
    if (m->gelu_tab) (void)hipFree(m->gelu_tab);
    for (auto mp : m->mlp_plans) if (mp) (void)ivit_mlp_plan_destroy(mp);
    for (auto pl : m->mlp_lin) if (pl) (void)ivit_linear_plan_destroy(pl);
    for (auto pl : m->lin_plans) if (pl) (void)ivit_linear_plan_destroy(pl);
    delete m;
    return IVIT_OK;
}

int ivit_swin_create(ivit_handle h, const ivit_swin_config *cfg, const ivit_swin_params *params, int max_slices,
                     ivit_swin *out) {
    CHECK_H(h);
    REQUIRE(h, cfg && params && out && params->blocks_host && params->dy_qact1, "null argument");
    REQUIRE(h, cfg->num_layers >= 1 && cfg->num_layers <= 4 && cfg->embed_dim > 0 && cfg->patch_size > 0 &&
                   cfg->img_size % cfg->patch_size == 0 && cfg->mlp_ratio > 0 && cfg->num_classes > 0,
            "bad model configuration");
    REQUIRE(h, cfg->num_layers == 1 || params->merges_host, "merges_host missing");
    REQUIRE(h, max_slices >= 1 && max_slices <= 16, "max_slices must be in [1, 16]");
    int nb = 0;
    const int grid = cfg->img_size / cfg->patch_size;
    if (cfg->window_size != 7 && cfg->window_size != 12) {
        snprintf(h->err, sizeof(h->err), "ivit_swin_create: built for windows 7 and 12 and head dim 32");
        return IVIT_ERR_UNSUPPORTED;
    }
    for (int li = 0; li < cfg->num_layers; ++li) {
        if (cfg->num_heads[li] <= 0 || ((cfg->embed_dim << li) / cfg->num_heads[li]) != 32 ||
            (cfg->embed_dim << li) % cfg->num_heads[li] != 0) {
            snprintf(h->err, sizeof(h->err), "ivit_swin_create: built for windows 7 and 12 and head dim 32");
            return IVIT_ERR_UNSUPPORTED;
        }
        nb += cfg->depths[li];
        // every stage resolution a multiple of the window, or at most the window (then one unshifted window of that
        // resolution, SwinTransformerBlock.__init__) whose size the fused attention is built for
        REQUIRE(h, (grid % (1 << li)) == 0, "every stage resolution must be a multiple of the window");
        const int res = grid >> li, wsz = res <= cfg->window_size ? res : cfg->window_size;
        REQUIRE(h, res % wsz == 0, "every stage resolution must be a multiple of the window");
        if (wsz != 7 && wsz != 12) {
            snprintf(h->err, sizeof(h->err), "ivit_swin_create: stage %d runs window %d; built for windows 7 and 12", li, wsz);
            return IVIT_ERR_UNSUPPORTED;
        }
    }
    REQUIRE(h, ((grid >> (cfg->num_layers - 1)) * (grid >> (cfg->num_layers - 1))) % 2 == 1 || params->s_pool > 0.f,
            "s_pool (the pool's input scale) is needed for an even final token count");
    ivit_swin_s *m = new (std::nothrow) ivit_swin_s();
    if (!m) return IVIT_ERR_HIP;
    m->h = h; m->cfg = *cfg; m->prm = *params;
    m->blocks.assign(params->blocks_host, params->blocks_host + nb);
    if (cfg->num_layers > 1) m->merges.assign(params->merges_host, params->merges_host + cfg->num_layers - 1);
    m->grid = grid; m->nblocks = nb; m->gelu_tab = nullptr; m->max_slices = max_slices;
    m->fused_mlp = true;
    if (hipMemcpy(&m->dy_qact1_host, params->dy_qact1, sizeof(ivit_dyadic), hipMemcpyDeviceToHost) != hipSuccess) {
        snprintf(h->err, sizeof(h->err), "ivit_swin_create: cannot read dy_qact1");
        delete m;
        return IVIT_ERR_HIP;
    }
    if (hipMalloc((void **)&m->gelu_tab, (size_t)nb * 65536) != hipSuccess) {
        snprintf(h->err, sizeof(h->err), "ivit_swin_create: hipMalloc failed");
        delete m;
        return IVIT_ERR_HIP;
    }
    for (int i = 0; i < nb; ++i) {
        int rc = ivit_shiftgelu_build_table(h, m->blocks[i].s_gelu, m->blocks[i].dy_gelu, gelu_table(m, i));
        if (rc != IVIT_OK) { ivit_swin_destroy(m); return rc; }
    }
    {   // fused Mlp plans for the C = 192 (hidden 768), C = 256 (hidden 1024) and C = 384 (hidden 1536) stages
        int bi = 0;
        for (int li = 0; li < cfg->num_layers; ++li)
            for (int bj = 0; bj < cfg->depths[li]; ++bj, ++bi) {
                const int C = cfg->embed_dim << li;
                ivit_linear_plan p1 = nullptr, p2 = nullptr;
                ivit_mlp_plan mp = nullptr;
                const ivit_swin_block &b = m->blocks[bi];
                if (mlp_plan_shape(C, cfg->mlp_ratio * C) &&
                    ivit_linear_plan_create(h, b.fc1.w, b.fc1.b, b.fc1.dy, 4 * C, C, &p1) == IVIT_OK &&
                    ivit_linear_plan_create(h, b.fc2.w, b.fc2.b, b.fc2.dy, C, 4 * C, &p2) == IVIT_OK) {
                    if (ivit_mlp_plan_create(h, p1, p2, &mp) != IVIT_OK) mp = nullptr;
                }
                m->mlp_lin.push_back(p1);
                m->mlp_lin.push_back(p2);
                m->mlp_plans.push_back(mp);
                // round 6: the C = 384 stage's qkv and proj layers on gemm_ws_qkv_kernel (prepared plans), norm1 inside the qkv launch.
                // (The kernel has a K = 192 geometry too, but with stage 1's qkv layer on it Swin-T b256 measured 1.1 % slower:
                // profiles/README.md, "Width 192 on the weights-in-registers GEMM")
                ivit_linear_plan q[2] = {nullptr, nullptr};
                if (C == Ws384Geo::K) {
                    if (ivit_linear_plan_create(h, b.qkv.w, b.qkv.b, b.qkv.dy, 3 * C, C, &q[0]) != IVIT_OK) q[0] = nullptr;
                    if (q[0] && ivit_linear_plan_prepare_ws(h, q[0]) != IVIT_OK) { (void)ivit_linear_plan_destroy(q[0]); q[0] = nullptr; }
                    if (ivit_linear_plan_create(h, b.proj.w, b.proj.b, b.proj.dy, C, C, &q[1]) != IVIT_OK) q[1] = nullptr;
                    if (q[1] && ivit_linear_plan_prepare_ws(h, q[1]) != IVIT_OK) { (void)ivit_linear_plan_destroy(q[1]); q[1] = nullptr; }
                }
                m->lin_plans.push_back(q[0]);
                m->lin_plans.push_back(q[1]);
            }
    }
    if (!m->run.create(h, max_slices)) {
        snprintf(h->err, sizeof(h->err), "ivit_swin_create: stream/event creation failed");
        ivit_swin_destroy(m);
        return IVIT_ERR_HIP;
    }
    *out = m;
    return IVIT_OK;
}

int ivit_swin_fused_mlp_blocks(ivit_swin m, int batch, int blocks_per_stage[4]) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE(m->h, blocks_per_stage && batch > 0, "bad arguments");
    int bi = 0;
    for (int li = 0; li < 4; ++li) {
        blocks_per_stage[li] = 0;
        if (li >= m->cfg.num_layers) continue;
        const int res = m->grid >> li;
        for (int bj = 0; bj < m->cfg.depths[li]; ++bj, ++bi)
            blocks_per_stage[li] += swin_mlp_mode(m, bi, m->cfg.embed_dim << li, (long long)batch * res * res) != 0;
    }
    return IVIT_OK;
}

}  // extern "C"

// =====================================================================================================
// The runner entries, once for both models: M is ivit_vit_s or ivit_swin_s.  A body reads in_chans, img_size and num_classes from
// m->cfg (both configurations spell them alike), the names in its refusals from `fn`, M::WS_ENTRY and M::FWD_ENTRY, and the rest
// through slice_stride, layout_images, num_features and run_slice
namespace {

template <class M>
size_t image_bytes(const M *m) { return (size_t)m->cfg.in_chans * m->cfg.img_size * m->cfg.img_size; }
template <class M>
size_t logit_bytes(const M *m, int batch) { return (size_t)batch * m->cfg.num_classes * 4; }

template <class M>
int workspace_bytes(M *m, int batch, int nslices, size_t *bytes) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE_FN(m->h, M::WS_ENTRY, bytes && batch > 0 && nslices >= 1 && nslices <= m->max_slices && nslices <= batch, "bad arguments");
    *bytes = slice_stride(m, max_slice(batch, nslices)) * (size_t)nslices;
    return IVIT_OK;
}

// the slice's view of what the caller asked for: the rows of every destination that belong to the batch's images b0 onward.  THE
// place a slice is placed in the caller's arrays (the planes of the hidden tap: RunOut::hid.rows, from the b0 set here)
template <class M>
RunOut slice_view(const M *m, const RunOut &all, int b0) {
    RunOut s = all;
    if (s.logits) s.logits += (size_t)b0 * m->cfg.num_classes;
    if (s.feat8) s.feat8 += (size_t)b0 * num_features(m);
    if (s.tok8) s.tok8 += (size_t)b0 * s.tok_image;
    if (s.attn.n) s.attn.attn16 += (size_t)b0 * s.attn.image;
    s.hid.b0 = (size_t)b0;
    return s;
}

// THE place a runner checks its arguments, and the order it does so in, before anything is launched: the workspace query, the
// pointers and the workspace's size and alignment, the three arrays of every runner pairwise; then the slices of the batch, each on
// its view of `out`, the whole batch's destinations as the entry filled them in.  Every entry with a forward in it ends here
template <class M>
int run_slices(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, const RunOut &out) {
    ivit_handle h = m->h;
    size_t need = 0;
    RUN(workspace_bytes(m, batch, nslices, &need));
    REQUIRE_FN(h, fn, images && out.any() && workspace && bytes >= need, "bad arguments / workspace too small");
    REQUIRE_FN(h, fn, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    const size_t img_bytes = image_bytes(m);
    const Extent a[3] = {{images, img_bytes * batch, "images", true}, {workspace, need, "workspace", false},
                         {out.logits, logit_bytes(m, batch), "logits", false}};
    RUN(extents_disjoint(h, fn, a, 0));
    const int Bmax = max_slice(batch, nslices);
    if (Bmax > max_slice_images(m)) {
        snprintf(h->err, sizeof(h->err), "%s: batch %d in %d slice(s) is %d images per slice, the model takes at most %d per slice: use more slices",
                 fn, batch, nslices, Bmax, max_slice_images(m));
        return IVIT_ERR_UNSUPPORTED;
    }
    const size_t stride = slice_stride(m, Bmax);
    return fork_join(m->run, h, batch, nslices, [&](ivit_handle sh, int i, int b0, int nb) {
        return run_slice(m, sh, images + (size_t)b0 * img_bytes, nb, layout_images(m, nb, Bmax), (char *)workspace + stride * (size_t)i,
                         slice_view(m, out, b0));
    });
}

template <class M>
int runner_forward(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits) {
    if (!m) return IVIT_ERR_INVALID;
    return run_slices(m, fn, images, batch, nslices, workspace, bytes, RunOut(logits));
}

// the forward, then the top-k of its logits on the handle's stream: behind the slices' join, so inside a capture it is one more node
template <class M>
int runner_predict(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                   const float *head_scale, int k, int32_t *idx, float *val) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE_FN(m->h, fn, head_scale && idx && k >= 1 && k <= TOPK_MAX_K && k <= m->cfg.num_classes,
               "head_scale / idx null or k outside 1 .. min(16, num_classes)");
    // idx / val against the forward's arrays and each other, judged BEFORE the forward is launched (ivit_logits_topk judges logits /
    // idx / val again behind it); a batch the workspace query refuses is left to the forward's own argument checks
    if (size_t need = 0; batch > 0 && workspace_bytes(m, batch, nslices, &need) == IVIT_OK) {
        const size_t nk = (size_t)batch * k * 4;
        const Extent a[5] = {{images, image_bytes(m) * batch, "images", true}, {workspace, need, "workspace", false},
                             {logits, logit_bytes(m, batch), "logits", false}, {idx, nk, "idx", false}, {val, nk, "val", false}};
        RUN(extents_disjoint(m->h, fn, a, 3));
    }
    RUN(runner_forward(m, M::FWD_ENTRY, images, batch, nslices, workspace, bytes, logits));
    return ivit_logits_topk(m->h, logits, head_scale, batch, m->cfg.num_classes, k, idx, val);
}

// the forward, then rank and nll of the labels among its logits (include/ivit_eval.h): the same place behind the slices' join
template <class M>
int runner_score(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                 const float *head_scale, const int64_t *labels, int32_t *rank, double *nll) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE_FN(m->h, fn, head_scale && labels && (rank || nll), "head_scale / labels null, or rank and nll both null");
    RUN(runner_forward(m, M::FWD_ENTRY, images, batch, nslices, workspace, bytes, logits));
    return ivit_logits_score(m->h, logits, head_scale, labels, batch, m->cfg.num_classes, rank, nll);
}

// forward_features (include/ivit_features.h): every argument checked first, then the slices with the caller's feat8 as the destination
// of the final norm (ViT) or the pool (Swin) — and the head only with logits —, then the fp32 form on the handle's stream, behind the
// slices' join
template <class M>
int runner_features(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                    int8_t *feat8, float scale, int mode, float *feat32) {
    if (!m) return IVIT_ERR_INVALID;
    RUN(features_args_ok(m->h, fn, feat8, num_features(m), scale, mode, feat32, true));
    RunOut out(logits);
    out.feat8 = feat8;
    RUN(run_slices(m, fn, images, batch, nslices, workspace, bytes, out));
    return feat32 ? ivit_features_f32(m->h, feat8, batch, num_features(m), scale, mode, feat32) : IVIT_OK;
}

}  // namespace

extern "C" {

// the nine runner entries of a model, written once and stamped for both: P is "ivit_vit" or "ivit_swin", the prefix of the entries and
// the handle type alike.  Each is one call of its shared body under its own name; a *_graph_create form captures the eager entry
#define RUNNER_ENTRIES(P) \
    int P##_workspace_bytes(P m, int batch, int nslices, size_t *bytes) { return workspace_bytes(m, batch, nslices, bytes); } \
    int P##_forward(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits) { \
        return runner_forward(m, __func__, images, batch, nslices, workspace, bytes, logits); \
    } \
    int P##_graph_create(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, ivit_graph *out) { \
        return graph_capture(m, out, P##_forward, images, batch, nslices, workspace, bytes, logits); \
    } \
    int P##_predict(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, \
                    const float *head_scale, int k, int32_t *idx, float *val) { \
        return runner_predict(m, __func__, images, batch, nslices, workspace, bytes, logits, head_scale, k, idx, val); \
    } \
    int P##_predict_graph_create(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, \
                                 const float *head_scale, int k, int32_t *idx, float *val, ivit_graph *out) { \
        return graph_capture(m, out, P##_predict, images, batch, nslices, workspace, bytes, logits, head_scale, k, idx, val); \
    } \
    int P##_score(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, \
                  const float *head_scale, const int64_t *labels, int32_t *rank, double *nll) { \
        return runner_score(m, __func__, images, batch, nslices, workspace, bytes, logits, head_scale, labels, rank, nll); \
    } \
    int P##_score_graph_create(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, \
                               const float *head_scale, const int64_t *labels, int32_t *rank, double *nll, ivit_graph *out) { \
        return graph_capture(m, out, P##_score, images, batch, nslices, workspace, bytes, logits, head_scale, labels, rank, nll); \
    } \
    int P##_features(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, int8_t *feat8, \
                     float scale, int mode, float *feat32) { \
        return runner_features(m, __func__, images, batch, nslices, workspace, bytes, logits, feat8, scale, mode, feat32); \
    } \
    int P##_features_graph_create(P m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits, \
                                  int8_t *feat8, float scale, int mode, float *feat32, ivit_graph *out) { \
        return graph_capture(m, out, P##_features, images, batch, nslices, workspace, bytes, logits, feat8, scale, mode, feat32); \
    }
RUNNER_ENTRIES(ivit_vit)
RUNNER_ENTRIES(ivit_swin)
#undef RUNNER_ENTRIES

// the class token's attention rows (include/ivit_attnmap.h), ViT only: every argument checked first — the block list, the fp32 map's
// rules, the five arrays pairwise (images / workspace / logits again in run_slices) —, then the slices with their taps, then the fp32 map
// on the handle's stream, behind the slices' join
int ivit_vit_attention(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                       const int *blocks_host, int nblocks, uint16_t *attn16, int mode, float *map32) {
    if (!m) return IVIT_ERR_INVALID;
    ivit_handle h = m->h;
    const int H = m->cfg.num_heads, T = m->T;
    RUN(index_list_ok(h, __func__, blocks_host, nblocks, "blocks_host", m->cfg.depth));
    RUN(attnmap_map_args_ok(h, __func__, attn16, "attn16", (long long)nblocks * std::max(batch, 0), H, T, mode, map32, "map32"));
    if (size_t need = 0; batch > 0 && workspace_bytes(m, batch, nslices, &need) == IVIT_OK) {
        const size_t rows = (size_t)nblocks * batch;
        const Extent a[5] = {{images, image_bytes(m) * batch, "images", true}, {workspace, need, "workspace", false},
                             {logits, logit_bytes(m, batch), "logits", false}, {attn16, rows * H * T * 2, "attn16", false},
                             {map32, attnmap_map_bytes((long long)rows, H, T, mode), "map32", false}};
        RUN(extents_disjoint(h, __func__, a, 3));
    }
    RUN(attnmap_shape_ok(h, __func__, T, m->cfg.embed_dim / H));
    if (map32 && H > ATTNMAP_MAX_H) {
        snprintf(h->err, sizeof(h->err), "%s: the fp32 map takes at most %d heads", __func__, ATTNMAP_MAX_H);
        return IVIT_ERR_UNSUPPORTED;
    }
    RunOut out(logits);
    out.attn.blocks = blocks_host; out.attn.n = nblocks; out.attn.attn16 = attn16;
    out.attn.image = (size_t)H * T; out.attn.plane = (size_t)std::max(batch, 0) * H * T;
    RUN(run_slices(m, __func__, images, batch, nslices, workspace, bytes, out));
    return map32 ? ivit_attention_map_f32(h, attn16, (int64_t)nblocks * batch, H, T, mode, map32) : IVIT_OK;
}
int ivit_vit_attention_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                                    const int *blocks_host, int nblocks, uint16_t *attn16, int mode, float *map32, ivit_graph *out) {
    return graph_capture(m, out, ivit_vit_attention, images, batch, nslices, workspace, bytes, logits, blocks_host, nblocks, attn16, mode, map32);
}

// class-activation maps (include/ivit_classmap.h), Swin only: every argument checked first — the mode and what it requires, the rules
// of ivit_class_map for the model's head and the caller's arrays, the eight arrays pairwise (images / workspace / logits again in
// run_slices) —, then the slices with the caller's tok8 as the destination of the final norm, then on the handle's stream, behind
// the slices' join, the top-k of the logits (TOPK mode) and the one launch of the maps
int ivit_swin_class_map(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                        const float *head_scale, int mode, int k, int32_t *idx, float *val, int8_t *tok8, const float *class_scale,
                        int32_t *cam32, float *map32) {
    if (!m) return IVIT_ERR_INVALID;
    ivit_handle h = m->h;
    const int L = final_tokens(m), C = num_features(m), ncls = m->cfg.num_classes;
    REQUIRE(h, mode == IVIT_CLASSMAP_TOPK || mode == IVIT_CLASSMAP_GIVEN, "mode must be IVIT_CLASSMAP_TOPK or IVIT_CLASSMAP_GIVEN");
    const bool given = mode == IVIT_CLASSMAP_GIVEN;
    if (given) REQUIRE(h, !val, "val must be null in IVIT_CLASSMAP_GIVEN mode (idx is the caller's)");
    else REQUIRE(h, logits && head_scale && k <= ncls, "IVIT_CLASSMAP_TOPK mode needs logits and head_scale, and k at most num_classes");
    REQUIRE_ALIGNED(h, val, "val", 4);
    RUN(classmap_args_ok(h, __func__, tok8, m->prm.head_w, idx, batch, L, C, ncls, k, class_scale, cam32, map32));
    if (size_t need = 0; workspace_bytes(m, batch, nslices, &need) == IVIT_OK) {
        const size_t nk = (size_t)batch * k * 4, nmap = nk * L;
        const Extent a[8] = {{images, image_bytes(m) * batch, "images", true}, {workspace, need, "workspace", false},
                             {logits, logit_bytes(m, batch), "logits", false}, {idx, nk, "idx", given}, {val, nk, "val", false},
                             {tok8, (size_t)batch * L * C, "tok8", false}, {cam32, nmap, "cam32", false}, {map32, nmap, "map32", false}};
        RUN(extents_disjoint(h, __func__, a, 3));       // images and the caller's idx: both only read
    }
    RunOut out(logits);
    out.tok8 = tok8; out.tok_image = (size_t)L * C;
    RUN(run_slices(m, __func__, images, batch, nslices, workspace, bytes, out));
    if (!given) RUN(ivit_logits_topk(h, logits, head_scale, batch, ncls, k, idx, val));
    return ivit_class_map(h, tok8, m->prm.head_w, idx, batch, L, C, ncls, k, class_scale, cam32, map32);
}
int ivit_swin_class_map_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                                     const float *head_scale, int mode, int k, int32_t *idx, float *val, int8_t *tok8,
                                     const float *class_scale, int32_t *cam32, float *map32, ivit_graph *out) {
    return graph_capture(m, out, ivit_swin_class_map, images, batch, nslices, workspace, bytes, logits, head_scale, mode, k, idx, val, tok8,
                         class_scale, cam32, map32);
}

}  // extern "C"

namespace {

// hidden states (include/ivit_hidden.h).  The scale of a site is a host float the model was created with: of a ViT block's output
// the next block's s_ln1 (s_ln behind the last), of a Swin stage's output the merge's s_in (s_norm_in behind the last stage)
inline float hidden_scale(const ivit_vit_s *m, int i) { return i + 1 < m->cfg.depth ? m->blocks[i + 1].s_ln1 : m->prm.s_ln; }
inline float hidden_scale(const ivit_swin_s *m, int s) { return s + 1 < m->cfg.num_layers ? m->merges[s].s_in : m->prm.s_norm_in; }

// both hidden_scale entries; `refusal`: the entry's own text
template <class M>
int runner_hidden_scale(M *m, const char *fn, int site, float *scale_host, const char *refusal) {
    if (!m) return IVIT_ERR_INVALID;
    REQUIRE_FN(m->h, fn, scale_host && site >= 0 && site < hidden_sites(m), refusal);
    *scale_host = hidden_scale(m, site);
    return IVIT_OK;
}

// both hidden_states entries: every argument checked first — the list, hid16, the layout, alignment, the planes' sizes, the rules of
// ivit_hidden_f32 for every plane, the five arrays pairwise (images / workspace / logits again in run_slices) —, then the slices with
// the caller's planes as the destination of the tapped blocks' last launches, then on the handle's stream, behind the slices' join,
// one ivit_hidden_f32 per plane.  `t0`: 1 drops the class row of a ViT's GRID form.  `list_name`: the list as the header spells it
template <class M>
int runner_hidden(M *m, const char *fn, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                  const int *list_host, int n, const char *list_name, int16_t *hid16, int layout, float *hid32, bool class_row) {
    if (!m) return IVIT_ERR_INVALID;
    ivit_handle h = m->h;
    RUN(index_list_ok(h, fn, list_host, n, list_name, hidden_sites(m)));
    REQUIRE_FN(h, fn, hid16, "hid16 is null");
    REQUIRE_FN(h, fn, !hid32 || layout == IVIT_HIDDEN_TOKENS || layout == IVIT_HIDDEN_GRID, "layout must be IVIT_HIDDEN_TOKENS or IVIT_HIDDEN_GRID");
    REQUIRE_FN(h, fn, ((uintptr_t)hid16 & 15) == 0, "hid16 must be 16-byte aligned");
    REQUIRE_FN(h, fn, ((uintptr_t)hid32 & 15) == 0, "hid32 must be 16-byte aligned");
    const int t0 = (class_row && hid32 && layout == IVIT_HIDDEN_GRID) ? 1 : 0;
    const size_t nb = (size_t)std::max(batch, 0);
    std::vector<size_t> at16(n + 1, 0), at32(n + 1, 0), image(n, 0);      // where plane j starts and what an image takes of it, in elements
    for (int j = 0; j < n; ++j) {
        const size_t T = hidden_tokens(m, list_host[j]), C = hidden_width(m, list_host[j]);
        // a slice's rows of a plane start b0 * T * C elements in: 16-byte aligned for every b0
        REQUIRE_FN(h, fn, (T * C) % 8 == 0, "the tokens times the width of a tapped plane must be a multiple of 8");
        at16[j + 1] = at16[j] + nb * T * C;
        at32[j + 1] = at32[j] + nb * (T - t0) * C;
        image[j] = T * C;
    }
    if (hid32 && batch > 0)
        for (int j = 0; j < n; ++j)
            RUN(hidden_args_ok(h, fn, hid16 + at16[j], "hid16", hidden_scale(m, list_host[j]), batch, hidden_tokens(m, list_host[j]),
                               hidden_width(m, list_host[j]), t0, layout, hid32 + at32[j], "hid32"));
    if (size_t need = 0; batch > 0 && workspace_bytes(m, batch, nslices, &need) == IVIT_OK) {
        const Extent a[5] = {{images, image_bytes(m) * batch, "images", true}, {workspace, need, "workspace", false},
                             {logits, logit_bytes(m, batch), "logits", false}, {hid16, at16[n] * 2, "hid16", false},
                             {hid32, at32[n] * 4, "hid32", false}};
        RUN(extents_disjoint(h, fn, a, 3));
    }
    RunOut out(logits);
    out.hid.idx = list_host; out.hid.n = n; out.hid.hid16 = hid16; out.hid.start = at16.data(); out.hid.image = image.data();
    RUN(run_slices(m, fn, images, batch, nslices, workspace, bytes, out));
    for (int j = 0; hid32 && j < n; ++j)
        RUN(ivit_hidden_f32(h, hid16 + at16[j], hidden_scale(m, list_host[j]), batch, hidden_tokens(m, list_host[j]), hidden_width(m, list_host[j]),
                            t0, layout, hid32 + at32[j]));
    return IVIT_OK;
}

}  // namespace

extern "C" {

int ivit_vit_hidden_scale(ivit_vit m, int block, float *scale_host) {
    return runner_hidden_scale(m, __func__, block, scale_host, "scale_host is null or block outside [0, depth)");
}
int ivit_swin_hidden_scale(ivit_swin m, int stage, float *scale_host) {
    return runner_hidden_scale(m, __func__, stage, scale_host, "scale_host is null or stage outside [0, num_layers)");
}

int ivit_vit_hidden_states(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                           const int *blocks_host, int nblocks, int16_t *hid16, int layout, float *hid32) {
    return runner_hidden(m, __func__, images, batch, nslices, workspace, bytes, logits, blocks_host, nblocks, "blocks_host", hid16, layout, hid32, true);
}
int ivit_vit_hidden_states_graph_create(ivit_vit m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                                        const int *blocks_host, int nblocks, int16_t *hid16, int layout, float *hid32, ivit_graph *out) {
    return graph_capture(m, out, ivit_vit_hidden_states, images, batch, nslices, workspace, bytes, logits, blocks_host, nblocks, hid16, layout, hid32);
}
int ivit_swin_hidden_states(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                            const int *stages_host, int nstages, int16_t *hid16, int layout, float *hid32) {
    return runner_hidden(m, __func__, images, batch, nslices, workspace, bytes, logits, stages_host, nstages, "stages_host", hid16, layout, hid32, false);
}
int ivit_swin_hidden_states_graph_create(ivit_swin m, const int8_t *images, int batch, int nslices, void *workspace, size_t bytes, int32_t *logits,
                                         const int *stages_host, int nstages, int16_t *hid16, int layout, float *hid32, ivit_graph *out) {
    return graph_capture(m, out, ivit_swin_hidden_states, images, batch, nslices, workspace, bytes, logits, stages_host, nstages, hid16, layout, hid32);
}

int ivit_graph_launch(ivit_graph g) {
    if (!g) return IVIT_ERR_INVALID;
    hipError_t e = hipGraphLaunch(g->exec, g->h->stream);
    if (e != hipSuccess) { snprintf(g->h->err, sizeof(g->h->err), "graph launch: %s", hipGetErrorString(e)); return IVIT_ERR_HIP; }
    return IVIT_OK;
}

int ivit_graph_destroy(ivit_graph g) {
    if (!g) return IVIT_ERR_INVALID;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return IVIT_OK;
}

}  // extern "C"

#undef RUN
#undef REQUIRE_FN
