// ivit_modelfile.h — frozen model files (include/ivit_modelfile.h): the reader and validator, the name -> field mapping of both models
// and the entries that turn a file into a live runner.
//
// Two halves.  The HOST half includes no HIP header and compiles with a plain host C++ compiler (tests/modelfile_harness.cpp builds it
// with sanitizers): mf::parse validates the bytes of a file, mf::fill_vit / mf::fill_swin are the name -> field mapping, written once in
// C as the counterpart of ivit_amd.engine.vit_native_params and ivit_amd.swin_engine.swin_native_params, and with it the check that
// every record the mapping reads is present with the dtype and shape the configuration implies; ivit_model_file_info is the entry on
// top of them.  The DEVICE half (not compiled with IVIT_MODELFILE_HOST_ONLY) is ivit_constants_checksum with its kernel, and
// ivit_model_open*: one allocation, the upload, the device checksum against the file's, the structs filled with blob + offset,
// ivit_*_create.
//
// The validator is the boundary to untrusted bytes: every offset, count and size is checked against the bytes actually present before
// it is used, counts are bounded before anything is allocated, names must be NUL-terminated within their field, and the tables are
// decoded ONCE into mf::File — nothing is read from the raw header a second time.  A little-endian host is assumed (the file is
// little-endian and fields are copied, not converted).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/ivit_modelfile.h"

namespace mf {

enum { HEADER = 256, RECORD = 96, SCALAR = 72, NAME = 48, MAX_COUNT = 65536, MAX_DIM = 1 << 20, MAX_DEPTH = 4096 };
enum { KIND_VIT = 1, KIND_SWIN = 2 };
enum { I1 = 1, U1 = 2, I2 = 3, U2 = 4, I4 = 5, F4 = 6, F8 = 7 };
enum { SC_F32 = 1, SC_DYADIC = 2, SC_I32 = 3 };
static const char *const DTYPE_NAME[8] = {"?", "i1", "u1", "i2", "u2", "i4", "f4", "f8"};
static const unsigned ITEM[8] = {0, 1, 1, 2, 2, 4, 4, 8};

struct Rec { const char *name; uint32_t dtype, rank; uint64_t shape[3], offset, bytes; };
struct Sca { const char *name; uint32_t kind; float f; double m, r; int32_t i; };
struct File {
    const uint8_t *data = nullptr; size_t size = 0;
    uint32_t format = 0, kind = 0, nrec = 0, nsca = 0;
    uint64_t file_bytes = 0, header_bytes = 0, blob_offset = 0, blob_bytes = 0, core_bytes = 0, header_sum = 0, blob_sum = 0;
    int32_t cfg[16] = {0};
    char cfg_name[64] = {0};
    std::vector<Rec> recs;
    std::vector<Sca> scas;
    const uint8_t *blob() const { return data + blob_offset; }
};
struct Err {
    int status = IVIT_OK;
    char msg[256] = {0};
    bool fail(int st, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
        status = st;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        return false;
    }
};
typedef unsigned long long ull;

// ---- the checksum (include/ivit_modelfile.h); `skip`: a byte offset whose 8-byte word is taken as 0 (the header's own sum), or -1
#ifdef __HIPCC__
#define IVIT_MF_HOST_DEVICE __host__ __device__
#else
#define IVIT_MF_HOST_DEVICE
#endif
IVIT_MF_HOST_DEVICE static inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline uint64_t checksum(const uint8_t *p, size_t n, long long skip = -1) {
    uint64_t sum = 0;
    const size_t words = n / 8;
    for (size_t i = 0; i < words; ++i) {
        uint64_t w;
        memcpy(&w, p + 8 * i, 8);
        if ((long long)(8 * i) == skip) w = 0;
        sum += mix64(w ^ ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull));
    }
    if (n % 8) {
        uint64_t w = 0;
        memcpy(&w, p + 8 * words, n % 8);
        sum += mix64(w ^ ((uint64_t)(words + 1) * 0x9E3779B97F4A7C15ull));
    }
    return sum;
}

template <class T> static inline T rd(const uint8_t *p) { T v; memcpy(&v, p, sizeof(T)); return v; }
static inline bool terminated(const uint8_t *p, size_t n) { return memchr(p, 0, n) != nullptr; }

static inline bool cfg_range(Err *e, const char *what, long long v, long long lo, long long hi) {
    return (v >= lo && v <= hi) || e->fail(IVIT_ERR_INVALID, "config: %s %lld is outside %lld .. %lld", what, v, lo, hi);
}

// ---- the configuration: bounded before anything is sized by it
static inline bool check_config(const File &f, Err *e) {
    const int32_t *c = f.cfg;
    static const char *const VIT[8] = {"img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "hidden_dim", "num_classes"};
    static const char *const SWIN[8] = {"img_size", "patch_size", "in_chans", "embed_dim", "num_layers", "window_size", "mlp_ratio", "num_classes"};
    if (f.kind == KIND_VIT) {
        if (!cfg_range(e, "depth", c[4], 1, MAX_DEPTH)) return false;
        for (int i = 0; i < 8; ++i) if (!cfg_range(e, VIT[i], c[i], 1, MAX_DIM)) return false;
        for (int i = 8; i < 16; ++i) if (c[i]) return e->fail(IVIT_ERR_INVALID, "config: unused field %d is %d, not 0", i, c[i]);
        if (c[0] % c[1]) return e->fail(IVIT_ERR_INVALID, "config: img_size %d is not a multiple of patch_size %d", c[0], c[1]);
        if (c[3] % c[5]) return e->fail(IVIT_ERR_INVALID, "config: embed_dim %d is not a multiple of num_heads %d", c[3], c[5]);
        if (c[0] / c[1] > 1024) return e->fail(IVIT_ERR_INVALID, "config: a grid of %d patches a side is outside 1 .. 1024", c[0] / c[1]);
        return true;
    }
    if (!cfg_range(e, "num_layers", c[4], 1, 4)) return false;
    for (int i = 0; i < 8; ++i) if (!cfg_range(e, SWIN[i], c[i], 1, i == 6 ? 64 : MAX_DIM)) return false;
    if (!cfg_range(e, "window_size", c[5], 1, 64)) return false;
    if (!cfg_range(e, "embed_dim", c[3], 1, MAX_DIM >> 4)) return false;
    for (int li = 0; li < 4; ++li) {
        if (li < c[4]) {
            if (!cfg_range(e, "depth", c[8 + li], 1, MAX_DEPTH) || !cfg_range(e, "num_heads", c[12 + li], 1, 1024)) return false;
            if ((c[3] << li) % c[12 + li]) return e->fail(IVIT_ERR_INVALID, "config: stage %d: width %d is not a multiple of num_heads %d", li, c[3] << li, c[12 + li]);
        } else if (c[8 + li] || c[12 + li]) {
            return e->fail(IVIT_ERR_INVALID, "config: stage %d is beyond num_layers %d but has depth %d and num_heads %d", li, c[4], c[8 + li], c[12 + li]);
        }
    }
    if (c[0] % c[1]) return e->fail(IVIT_ERR_INVALID, "config: img_size %d is not a multiple of patch_size %d", c[0], c[1]);
    if ((c[0] / c[1]) % (1 << (c[4] - 1)) || c[0] / c[1] > 4096)
        return e->fail(IVIT_ERR_INVALID, "config: a grid of %d patches a side does not halve %d times", c[0] / c[1], c[4] - 1);
    return true;
}

// ---- bytes -> File: structure, both checksums.  `data` must stay valid while the File is used (names point into it)
static inline bool parse(const uint8_t *data, size_t size, File *f, Err *e) {
    const int INV = IVIT_ERR_INVALID;
    if (!data || size < HEADER) return e->fail(INV, "header: file holds %llu bytes, fewer than the %d of the fixed header", (ull)size, HEADER);
    if (memcmp(data, "IVITMDL\0", 8) != 0) return e->fail(INV, "header: bad magic");
    f->data = data; f->size = size;
    f->format = rd<uint32_t>(data + 8); f->kind = rd<uint32_t>(data + 12);
    if (f->format == 0) return e->fail(INV, "header: format version 0");
    if (f->format > 1) return e->fail(IVIT_ERR_UNSUPPORTED, "header: format version %u is newer than 1", f->format);
    if (f->kind != KIND_VIT && f->kind != KIND_SWIN) return e->fail(IVIT_ERR_UNSUPPORTED, "header: unknown kind %u", f->kind);
    f->file_bytes = rd<uint64_t>(data + 16); f->header_bytes = rd<uint64_t>(data + 24); f->blob_offset = rd<uint64_t>(data + 32);
    f->blob_bytes = rd<uint64_t>(data + 40); f->core_bytes = rd<uint64_t>(data + 48);
    f->nrec = rd<uint32_t>(data + 56); f->nsca = rd<uint32_t>(data + 60);
    f->header_sum = rd<uint64_t>(data + 64); f->blob_sum = rd<uint64_t>(data + 72);
    if (f->file_bytes != size) return e->fail(INV, "header: file holds %llu bytes, its header says %llu", (ull)size, (ull)f->file_bytes);
    if (f->blob_offset < HEADER || f->blob_offset > size || f->blob_offset % 256)
        return e->fail(INV, "header: blob offset %llu is not a multiple of 256 inside the file of %llu bytes", (ull)f->blob_offset, (ull)size);
    if (f->blob_bytes != size - f->blob_offset)
        return e->fail(INV, "header: blob of %llu bytes at offset %llu does not end with the file of %llu bytes", (ull)f->blob_bytes, (ull)f->blob_offset, (ull)size);
    if (f->core_bytes > f->blob_bytes || f->core_bytes % 256)
        return e->fail(INV, "header: core size %llu is not a multiple of 256 within the blob of %llu bytes", (ull)f->core_bytes, (ull)f->blob_bytes);
    const uint64_t hsum = checksum(data, (size_t)f->blob_offset, 64);
    if (hsum != f->header_sum) return e->fail(INV, "header: checksum %016llx, the header says %016llx", (ull)hsum, (ull)f->header_sum);
    if (f->nrec > MAX_COUNT) return e->fail(INV, "records: count %u exceeds %d", f->nrec, MAX_COUNT);
    if (f->nsca > MAX_COUNT) return e->fail(INV, "scalars: count %u exceeds %d", f->nsca, MAX_COUNT);
    const uint64_t tables_end = HEADER + (uint64_t)RECORD * f->nrec + (uint64_t)SCALAR * f->nsca;       // < 2^24: the counts are bounded
    if (f->header_bytes != tables_end || f->blob_offset != (tables_end + 255) / 256 * 256)
        return e->fail(INV, "header: tables of %u records and %u scalars end at %llu, the header says %llu and the blob starts at %llu", f->nrec,
                       f->nsca, (ull)tables_end, (ull)f->header_bytes, (ull)f->blob_offset);
    for (size_t i = 208; i < HEADER; ++i) if (data[i]) return e->fail(INV, "header: reserved byte %llu is not 0", (ull)i);
    for (uint64_t i = tables_end; i < f->blob_offset; ++i) if (data[i]) return e->fail(INV, "header: padding byte %llu is not 0", (ull)i);
    for (int i = 0; i < 16; ++i) f->cfg[i] = rd<int32_t>(data + 80 + 4 * i);
    if (!terminated(data + 144, 64)) return e->fail(INV, "config: name is not terminated");
    memcpy(f->cfg_name, data + 144, 64);
    if (!check_config(*f, e)) return false;

    f->recs.resize(f->nrec);
    for (uint32_t i = 0; i < f->nrec; ++i) {
        const uint8_t *p = data + HEADER + (size_t)RECORD * i;
        Rec &r = f->recs[i];
        if (!terminated(p, NAME) || !p[0]) return e->fail(INV, "records: record %u: name is empty or not terminated", i);
        r.name = (const char *)p;
        r.dtype = rd<uint32_t>(p + 48); r.rank = rd<uint32_t>(p + 52);
        for (int d = 0; d < 3; ++d) r.shape[d] = rd<uint64_t>(p + 56 + 8 * d);
        r.offset = rd<uint64_t>(p + 80); r.bytes = rd<uint64_t>(p + 88);
        if (i) {
            const int c = strcmp(f->recs[i - 1].name, r.name);
            if (c == 0) return e->fail(INV, "records: record %u \"%s\": duplicate name", i, r.name);
            if (c > 0) return e->fail(INV, "records: record %u \"%s\": names are not sorted", i, r.name);
        }
        if (r.dtype < 1 || r.dtype > 7) return e->fail(INV, "records: record %u \"%s\": unknown dtype code %u", i, r.name, r.dtype);
        if (r.rank < 1 || r.rank > 3) return e->fail(INV, "records: record %u \"%s\": rank %u is outside 1 .. 3", i, r.name, r.rank);
        uint64_t want = ITEM[r.dtype];
        for (uint32_t d = 0; d < 3; ++d) {
            if (d >= r.rank) {
                if (r.shape[d]) return e->fail(INV, "records: record %u \"%s\": unused dimension %u is %llu, not 0", i, r.name, d, (ull)r.shape[d]);
                continue;
            }
            if (r.shape[d] < 1 || r.shape[d] > (1ull << 32) || want > (1ull << 62) / r.shape[d])
                return e->fail(INV, "records: record %u \"%s\": dimension %u is %llu", i, r.name, d, (ull)r.shape[d]);
            want *= r.shape[d];
        }
        if (r.bytes != want) return e->fail(INV, "records: record %u \"%s\": %llu bytes, its shape and dtype give %llu", i, r.name, (ull)r.bytes, (ull)want);
        if (r.offset % 256) return e->fail(INV, "records: record %u \"%s\": offset %llu is not a multiple of 256", i, r.name, (ull)r.offset);
        if (r.bytes > f->blob_bytes || r.offset > f->blob_bytes - r.bytes)
            return e->fail(INV, "records: record %u \"%s\": offset %llu + %llu bytes passes the blob of %llu", i, r.name, (ull)r.offset, (ull)r.bytes,
                           (ull)f->blob_bytes);
        if (r.offset < f->core_bytes && r.offset + r.bytes > f->core_bytes)
            return e->fail(INV, "records: record %u \"%s\": offset %llu + %llu bytes crosses the core size %llu", i, r.name, (ull)r.offset, (ull)r.bytes,
                           (ull)f->core_bytes);
    }
    {   // overlaps: by offset
        std::vector<uint32_t> order(f->nrec);
        for (uint32_t i = 0; i < f->nrec; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return f->recs[a].offset != f->recs[b].offset ? f->recs[a].offset < f->recs[b].offset : a < b; });
        for (uint32_t j = 1; j < f->nrec; ++j) {
            const Rec &a = f->recs[order[j - 1]], &b = f->recs[order[j]];
            if (a.offset + a.bytes > b.offset) return e->fail(INV, "records: records \"%s\" and \"%s\" overlap at offset %llu", a.name, b.name, (ull)b.offset);
        }
    }
    f->scas.resize(f->nsca);
    for (uint32_t i = 0; i < f->nsca; ++i) {
        const uint8_t *p = data + HEADER + (size_t)RECORD * f->nrec + (size_t)SCALAR * i;
        Sca &s = f->scas[i];
        if (!terminated(p, NAME) || !p[0]) return e->fail(INV, "scalars: scalar %u: name is empty or not terminated", i);
        s.name = (const char *)p;
        s.kind = rd<uint32_t>(p + 48);
        if (i) {
            const int c = strcmp(f->scas[i - 1].name, s.name);
            if (c == 0) return e->fail(INV, "scalars: scalar %u \"%s\": duplicate name", i, s.name);
            if (c > 0) return e->fail(INV, "scalars: scalar %u \"%s\": names are not sorted", i, s.name);
        }
        if (s.kind < 1 || s.kind > 3) return e->fail(INV, "scalars: scalar %u \"%s\": unknown kind %u", i, s.name, s.kind);
        s.f = 0.f; s.m = s.r = 0.0; s.i = 0;
        if (s.kind == SC_F32) s.f = rd<float>(p + 56);
        if (s.kind == SC_DYADIC) { s.m = rd<double>(p + 56); s.r = rd<double>(p + 64); }
        if (s.kind == SC_I32) s.i = rd<int32_t>(p + 56);
        const size_t used = s.kind == SC_DYADIC ? 16 : 4;
        for (size_t b = 52; b < SCALAR; ++b)
            if ((b < 56 || b >= 56 + used) && p[b]) return e->fail(INV, "scalars: scalar %u \"%s\": unused byte %llu is not 0", i, s.name, (ull)b);
    }
    const uint64_t bsum = checksum(f->blob(), (size_t)f->blob_bytes);
    if (bsum != f->blob_sum) return e->fail(INV, "blob: checksum %016llx, the header says %016llx", (ull)bsum, (ull)f->blob_sum);
    return true;
}

static inline const Rec *find_record(const File &f, const char *name) {
    auto it = std::lower_bound(f.recs.begin(), f.recs.end(), name, [](const Rec &r, const char *n) { return strcmp(r.name, n) < 0; });
    return it != f.recs.end() && strcmp(it->name, name) == 0 ? &*it : nullptr;
}
static inline const Sca *find_scalar(const File &f, const char *name) {
    auto it = std::lower_bound(f.scas.begin(), f.scas.end(), name, [](const Sca &s, const char *n) { return strcmp(s.name, n) < 0; });
    return it != f.scas.end() && strcmp(it->name, name) == 0 ? &*it : nullptr;
}

// ---- the name -> field mapping.  A Fill hands out `base + offset` of a record after checking its dtype and shape, and the scalars;
// the first problem is kept in the Err and everything after it returns zeros.  base = 0 validates without a device
struct Fill {
    const File &f; uintptr_t base; Err *e; bool ok = true;
    char nm[96] = {0};
    const char *name(const char *prefix, const char *leaf) { snprintf(nm, sizeof(nm), "%s%s", prefix, leaf); return nm; }
    bool has(const char *prefix, const char *leaf) { return find_record(f, name(prefix, leaf)) != nullptr; }
    bool has_scalar(const char *prefix, const char *leaf) { return find_scalar(f, name(prefix, leaf)) != nullptr; }
    const Rec *rec(const char *prefix, const char *leaf, uint32_t dtype, uint32_t rank, uint64_t d0, uint64_t d1 = 0, uint64_t d2 = 0) {
        if (!ok) return nullptr;
        const Rec *r = find_record(f, name(prefix, leaf));
        if (!r) { ok = e->fail(IVIT_ERR_INVALID, "model: record \"%s\" is missing", nm); return nullptr; }
        if (r->dtype != dtype || r->rank != rank || r->shape[0] != d0 || r->shape[1] != d1 || r->shape[2] != d2) {
            ok = e->fail(IVIT_ERR_INVALID, "model: record \"%s\" is %s [%llu, %llu, %llu], the configuration implies %s [%llu, %llu, %llu]", nm,
                         DTYPE_NAME[r->dtype], (ull)r->shape[0], (ull)r->shape[1], (ull)r->shape[2], DTYPE_NAME[dtype], (ull)d0, (ull)d1, (ull)d2);
            return nullptr;
        }
        return r;
    }
    template <class T> const T *ptr(const char *prefix, const char *leaf, uint32_t dtype, uint32_t rank, uint64_t d0, uint64_t d1 = 0, uint64_t d2 = 0) {
        const Rec *r = rec(prefix, leaf, dtype, rank, d0, d1, d2);
        return r ? (const T *)(base + (uintptr_t)r->offset) : nullptr;
    }
    const ivit_dyadic *dy_table(const char *prefix, const char *leaf, uint64_t n) { return ptr<ivit_dyadic>(prefix, leaf, F8, 2, n, 2); }
    // a by-value dyadic of a ViT: a float64 [1, 2] record, read from the host copy of the blob (ivit_amd.engine.host_scalars)
    ivit_dyadic dy_blob(const char *prefix, const char *leaf) {
        ivit_dyadic d = {0.0, 0.0};
        if (const Rec *r = rec(prefix, leaf, F8, 2, 1, 2)) memcpy(&d, f.blob() + r->offset, 16);
        return d;
    }
    const Sca *scalar(const char *prefix, const char *leaf, uint32_t kind) {
        if (!ok) return nullptr;
        const Sca *s = find_scalar(f, name(prefix, leaf));
        if (!s) { ok = e->fail(IVIT_ERR_INVALID, "model: scalar \"%s\" is missing", nm); return nullptr; }
        if (s->kind != kind) { ok = e->fail(IVIT_ERR_INVALID, "model: scalar \"%s\" has kind %u, not %u", nm, s->kind, kind); return nullptr; }
        return s;
    }
    float f32(const char *prefix, const char *leaf) { const Sca *s = scalar(prefix, leaf, SC_F32); return s ? s->f : 0.f; }
    ivit_dyadic dy(const char *prefix, const char *leaf) {
        const Sca *s = scalar(prefix, leaf, SC_DYADIC);
        ivit_dyadic d = {s ? s->m : 0.0, s ? s->r : 0.0};
        return d;
    }
    void ln(const char *prefix, uint64_t C, const float **bias_int, const float **sc, const ivit_dyadic **dyp) {
        char p[sizeof(nm)];                      // a copy: `prefix` may be nm itself
        snprintf(p, sizeof(p), "%s", prefix);
        *bias_int = ptr<float>(p, ".bias_int", F4, 1, C); *sc = ptr<float>(p, ".sc", F4, 1, C); *dyp = dy_table(p, ".dy", C);
    }
    void lin(const char *prefix, uint64_t N, uint64_t K, bool bias, const int8_t **w, const int32_t **b, const ivit_dyadic **dyp) {
        char p[sizeof(nm)];                      // a copy: `prefix` may be nm itself
        snprintf(p, sizeof(p), "%s", prefix);
        *w = ptr<int8_t>(p, ".w", I1, 2, N, K);
        *b = bias ? ptr<int32_t>(p, ".b", I4, 1, N) : nullptr;
        if (dyp) *dyp = dy_table(p, ".dy", N);
    }
    // the optional Shiftmax tables of one attention: all of their records or none.  (nc, tcount) size the records
    template <class B> void exp_tables(const char *p, B *b, bool present, int nc, int tcount, int dmin) {
        if (!present || !ok) return;
        if (nc < 1 || nc > 256 || tcount < 1 || tcount > 65535 || dmin > 0 || dmin < -255) {
            ok = e->fail(IVIT_ERR_INVALID, "model: Shiftmax tables of \"%sattn\": metadata (%d, %d, %d) is out of range", p, nc, tcount, dmin);
            return;
        }
        b->exp_aq = ptr<uint16_t>(p, "attn.exp_aq", U2, 2, (uint64_t)nc, 256);
        b->exp_t = ptr<float>(p, "attn.exp_t", F4, 1, (uint64_t)tcount);
        b->exp_cls = ptr<uint8_t>(p, "attn.exp_cls", U1, 1, 256);
        b->exp_nc = nc; b->exp_tcount = tcount; b->exp_dmin = dmin;
    }
};

// ivit_amd.engine.vit_native_params
static inline bool fill_vit(const File &f, uintptr_t base, ivit_vit_config *cfg, ivit_vit_params *prm, std::vector<ivit_vit_block> *blocks, Err *e) {
    Fill F{f, base, e};
    const int32_t *c = f.cfg;
    const ivit_vit_config k = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
    *cfg = k;
    const uint64_t D = k.embed_dim, Hd = k.hidden_dim, NC = k.num_classes, g = k.img_size / k.patch_size, T = g * g + 1;
    const uint64_t Kp = (uint64_t)k.in_chans * k.patch_size * k.patch_size;
    blocks->assign(k.depth, ivit_vit_block());
    for (int i = 0; i < k.depth && F.ok; ++i) {
        char p[32];
        snprintf(p, sizeof(p), "blocks.%d.", i);
        ivit_vit_block &b = (*blocks)[i];
        memset(&b, 0, sizeof(b));
        b.s_ln1 = F.f32(p, "ln1.s");
        F.ln(F.name(p, "norm1"), D, &b.n1_bias_int, &b.n1_sc, &b.n1_dy);
        F.lin(F.name(p, "attn.qkv"), 3 * D, D, true, &b.qkv_w, &b.qkv_b, &b.qkv_dy);
        b.dy_qk = F.dy_blob(p, "attn.dy_qk"); b.s_softmax = F.f32(p, "attn.s_softmax"); b.dy_pv = F.dy_blob(p, "attn.dy_pv");
        const int have = F.has(p, "attn.exp_meta") + F.has(p, "attn.exp_aq") + F.has(p, "attn.exp_t") + F.has(p, "attn.exp_cls");
        if (have != 0 && have != 4 && F.ok) F.ok = e->fail(IVIT_ERR_INVALID, "model: Shiftmax tables of \"%sattn\" are partly present (%d of 4 records)", p, have);
        if (have == 4) {
            int32_t meta[3] = {0, 0, 0};
            if (const Rec *r = F.rec(p, "attn.exp_meta", I4, 1, 3)) memcpy(meta, f.blob() + r->offset, 12);
            F.exp_tables(p, &b, true, meta[0], meta[1], meta[2]);
        }
        F.lin(F.name(p, "attn.proj"), D, D, true, &b.proj_w, &b.proj_b, &b.proj_dy);
        b.res1_main = F.dy_blob(p, "res1.dy_main"); b.res1_res = F.dy_blob(p, "res1.dy_res");
        b.s_ln2 = F.f32(p, "ln2.s");
        F.ln(F.name(p, "norm2"), D, &b.n2_bias_int, &b.n2_sc, &b.n2_dy);
        F.lin(F.name(p, "mlp.fc1"), Hd, D, true, &b.fc1_w, &b.fc1_b, &b.fc1_dy);
        b.s_gelu = F.f32(p, "mlp.s_gelu"); b.dy_gelu = F.dy_blob(p, "mlp.dy_gelu");
        F.lin(F.name(p, "mlp.fc2"), D, Hd, true, &b.fc2_w, &b.fc2_b, &b.fc2_dy);
        b.res2_main = F.dy_blob(p, "res2.dy_main"); b.res2_res = F.dy_blob(p, "res2.dy_res");
    }
    memset(prm, 0, sizeof(*prm));
    F.lin("patch_embed.proj", D, Kp, true, &prm->pe_w, &prm->pe_b, &prm->pe_dy);
    prm->z_cls = F.ptr<int32_t>("", "z_cls", I4, 1, D); prm->pos = F.ptr<int16_t>("", "pos", I2, 2, T, D);
    prm->dy_x = F.dy_blob("", "embed.dy_x"); prm->dy_pos = F.dy_blob("", "embed.dy_pos");
    prm->blocks_host = blocks->data();
    prm->s_ln = F.f32("", "ln.s");
    F.ln("norm", D, &prm->n_bias_int, &prm->n_sc, &prm->n_dy);
    F.lin("head", NC, D, true, &prm->head_w, &prm->head_b, nullptr);
    F.ptr<float>("", "head.scale", F4, 1, NC);
    F.f32("", "input.s"); F.f32("", "feat.s");
    return F.ok;
}

// ivit_amd.swin_engine.swin_native_params
static inline bool fill_swin(const File &f, uintptr_t base, ivit_swin_config *cfg, ivit_swin_params *prm, std::vector<ivit_swin_block> *blocks,
                             std::vector<ivit_swin_merge> *merges, Err *e) {
    Fill F{f, base, e};
    const int32_t *c = f.cfg;
    memset(cfg, 0, sizeof(*cfg));
    cfg->img_size = c[0]; cfg->patch_size = c[1]; cfg->in_chans = c[2]; cfg->embed_dim = c[3]; cfg->num_layers = c[4];
    cfg->window_size = c[5]; cfg->mlp_ratio = c[6]; cfg->num_classes = c[7];
    size_t nb = 0;
    for (int li = 0; li < 4; ++li) { cfg->depths[li] = c[8 + li]; cfg->num_heads[li] = c[12 + li]; nb += (size_t)c[8 + li]; }
    const uint64_t E = cfg->embed_dim, NC = cfg->num_classes, R = cfg->mlp_ratio, grid = cfg->img_size / cfg->patch_size;
    const uint64_t Kp = (uint64_t)cfg->in_chans * cfg->patch_size * cfg->patch_size;
    blocks->assign(nb, ivit_swin_block());
    merges->assign(cfg->num_layers > 1 ? cfg->num_layers - 1 : 1, ivit_swin_merge());
    size_t i = 0;
    for (int li = 0; li < cfg->num_layers && F.ok; ++li) {
        const uint64_t C = E << li, heads = cfg->num_heads[li], res = grid >> li, ws = std::min<uint64_t>(cfg->window_size, res), N = ws * ws;
        for (int bj = 0; bj < cfg->depths[li] && F.ok; ++bj, ++i) {
            char p[48];
            snprintf(p, sizeof(p), "layers.%d.blocks.%d.", li, bj);
            ivit_swin_block &b = (*blocks)[i];
            memset(&b, 0, sizeof(b));
            b.s_in = F.f32(p, "s_in");
            F.ln(F.name(p, "norm1"), C, &b.n1.bias_int, &b.n1.sc, &b.n1.dy);
            F.lin(F.name(p, "attn.qkv"), 3 * C, C, true, &b.qkv.w, &b.qkv.b, &b.qkv.dy);
            b.dy_qk = F.dy(p, "attn.dy_qk"); b.dy_a = F.dy(p, "attn.dy_a");
            b.relb = F.ptr<int16_t>(p, "attn.relb", I2, 3, heads, N, N);
            b.s_softmax = F.f32(p, "attn.s_softmax"); b.dy_pv = F.dy(p, "attn.dy_pv");
            F.lin(F.name(p, "attn.proj"), C, C, true, &b.proj.w, &b.proj.b, &b.proj.dy);
            const int have = F.has(p, "attn.exp_aq") + F.has(p, "attn.exp_t") + F.has(p, "attn.exp_cls");
            const int meta = F.has_scalar(p, "attn.exp_nc") + F.has_scalar(p, "attn.exp_tcount") + F.has_scalar(p, "attn.exp_dmin");
            if (((have != 0 && have != 3) || meta != have) && F.ok)
                F.ok = e->fail(IVIT_ERR_INVALID, "model: Shiftmax tables of \"%sattn\" are partly present (%d of 3 records, %d of 3 scalars)", p, have, meta);
            if (have == 3) {
                const float nc = F.f32(p, "attn.exp_nc"), tc = F.f32(p, "attn.exp_tcount"), dm = F.f32(p, "attn.exp_dmin");
                const bool sane = nc >= 0 && nc <= 65536 && tc >= 0 && tc <= 65536 && dm >= -65536 && dm <= 65536;     // also refuses NaN
                F.exp_tables(p, &b, true, sane ? (int)nc : -1, sane ? (int)tc : -1, sane ? (int)dm : 1);
            }
            b.res1_main = F.dy(p, "res1.dy_main"); b.res1_res = F.dy(p, "res1.dy_res");
            b.s_mid = F.f32(p, "s_mid");
            F.ln(F.name(p, "norm2"), C, &b.n2.bias_int, &b.n2.sc, &b.n2.dy);
            F.lin(F.name(p, "mlp.fc1"), R * C, C, true, &b.fc1.w, &b.fc1.b, &b.fc1.dy);
            b.s_gelu = F.f32(p, "mlp.s_gelu"); b.dy_gelu = F.dy(p, "mlp.dy_gelu");
            F.lin(F.name(p, "mlp.fc2"), C, R * C, true, &b.fc2.w, &b.fc2.b, &b.fc2.dy);
            b.res2_main = F.dy(p, "res2.dy_main"); b.res2_res = F.dy(p, "res2.dy_res");
        }
        if (li < cfg->num_layers - 1) {
            char p[48];
            snprintf(p, sizeof(p), "layers.%d.downsample.", li);
            ivit_swin_merge &g = (*merges)[li];
            memset(&g, 0, sizeof(g));
            g.s_in = F.f32(p, "s_in");
            F.ln(F.name(p, "norm"), 4 * C, &g.n.bias_int, &g.n.sc, &g.n.dy);
            F.lin(F.name(p, "reduction"), 2 * C, 4 * C, false, &g.red.w, &g.red.b, &g.red.dy);
        }
    }
    const uint64_t CL = E << (cfg->num_layers - 1);
    memset(prm, 0, sizeof(*prm));
    F.lin("patch_embed.proj", E, Kp, true, &prm->pe.w, &prm->pe.b, &prm->pe.dy);
    prm->s_bn = F.f32("", "patch_embed.s_bn");
    F.ln("patch_embed.norm", E, &prm->pn.bias_int, &prm->pn.sc, &prm->pn.dy);
    prm->dy_qact1 = F.dy_table("", "dy_qact1", 1);
    prm->blocks_host = blocks->data();
    prm->merges_host = merges->data();
    prm->s_norm_in = F.f32("", "norm.s_in");
    F.ln("norm", CL, &prm->n.bias_int, &prm->n.sc, &prm->n.dy);
    prm->dy_pool = F.dy("", "dy_pool");
    F.lin("head", NC, CL, true, &prm->head_w, &prm->head_b, nullptr);
    prm->s_pool = F.f32("", "pool.s_in");
    F.ptr<float>("", "head.scale", F4, 1, NC);
    F.ptr<float>("", "class_scale", F4, 1, NC);
    F.f32("", "input.s"); F.f32("", "feat.s");
    return F.ok;
}

// structure, checksums and the mapping, without a device: what ivit_model_file_info and the first step of ivit_model_open share
static inline bool validate(const uint8_t *data, size_t size, File *f, Err *e) {
    if (!parse(data, size, f, e)) return false;
    if (f->kind == KIND_VIT) {
        ivit_vit_config c; ivit_vit_params p; std::vector<ivit_vit_block> b;
        return fill_vit(*f, 0, &c, &p, &b, e);
    }
    ivit_swin_config c; ivit_swin_params p; std::vector<ivit_swin_block> b; std::vector<ivit_swin_merge> g;
    return fill_swin(*f, 0, &c, &p, &b, &g, e);
}

static inline void info_of(const File &f, ivit_model_info *info) {
    memset(info, 0, sizeof(*info));
    info->format = (int)f.format; info->kind = (int)f.kind;
    info->img_size = f.cfg[0]; info->in_chans = f.cfg[2]; info->num_classes = f.cfg[7];
    info->num_features = f.kind == KIND_VIT ? f.cfg[3] : f.cfg[3] << (f.cfg[4] - 1);
    info->records = (int)f.nrec; info->scalars = (int)f.nsca;
    info->file_bytes = (int64_t)f.file_bytes; info->blob_bytes = (int64_t)f.blob_bytes;
    const Sca *a = find_scalar(f, "input.s"), *b = find_scalar(f, "feat.s");
    info->s_input = a ? a->f : 0.f; info->s_features = b ? b->f : 0.f;
}

// the whole file into memory; refuses what it cannot read completely
static inline bool read_file(const char *path, std::vector<uint8_t> *out, Err *e) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return e->fail(IVIT_ERR_INVALID, "file: cannot open \"%s\"", path);
    bool ok = fseek(fp, 0, SEEK_END) == 0;
    const long long n = ok ? (long long)ftell(fp) : -1;
    ok = ok && n >= 0 && n <= (1ll << 40) && fseek(fp, 0, SEEK_SET) == 0;
    if (ok) {
        try { out->resize((size_t)n); } catch (...) { ok = false; }           // a file larger than memory is refused, not thrown through C
        ok = ok && (n == 0 || fread(out->data(), 1, (size_t)n, fp) == (size_t)n);
    }
    fclose(fp);
    return ok || e->fail(IVIT_ERR_INVALID, "file: cannot read \"%s\"", path);
}

}  // namespace mf

extern "C" int ivit_model_file_info(const char *path, ivit_model_info *info, char *msg, size_t msg_bytes) {
    if (msg && msg_bytes) msg[0] = 0;
    if (info) memset(info, 0, sizeof(*info));
    mf::Err e;
    std::vector<uint8_t> bytes;
    mf::File f;
    if (!path || !info) e.fail(IVIT_ERR_INVALID, "ivit_model_file_info: path or info is null");
    else if (mf::read_file(path, &bytes, &e) && mf::validate(bytes.data(), bytes.size(), &f, &e)) mf::info_of(f, info);
    if (e.status != IVIT_OK && msg && msg_bytes) snprintf(msg, msg_bytes, "%s", e.msg);
    return e.status;
}

#ifndef IVIT_MODELFILE_HOST_ONLY
// ================================================================ the device half

// ---- the checksum over device memory.  A grid-stride pass over 16-byte pieces (one global_load_dwordx4 per lane and step), per-lane
// 64-bit partial sums; the tail of fewer than 16 bytes is assembled byte by byte by one thread and never read beyond `bytes`; the
// partials are summed over the wavefront by shuffles, over the workgroup through LDS, and one atomic add per workgroup lands in *sum.
// Integer addition mod 2^64 is associative and commutative, so the result does not depend on the order
#define CHECKSUM_THREADS 256
__global__ __launch_bounds__(CHECKSUM_THREADS) void constants_checksum_kernel(const uint8_t *__restrict__ p, size_t bytes, unsigned long long *__restrict__ sum) {
    const size_t pieces = bytes / 16, stride = (size_t)gridDim.x * CHECKSUM_THREADS;
    const unsigned long long K = 0x9E3779B97F4A7C15ull;
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * CHECKSUM_THREADS + threadIdx.x; i < pieces; i += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
        const unsigned long long w0 = (unsigned long long)v.x | ((unsigned long long)v.y << 32), w1 = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
        acc += mf::mix64(w0 ^ ((2 * i + 1) * K)) + mf::mix64(w1 ^ ((2 * i + 2) * K));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t done = pieces * 16, tail = bytes - done;           // 0 .. 15 bytes: at most two words, the second partial
        for (size_t w = 0; w * 8 < tail; ++w) {
            unsigned long long word = 0;
            const size_t n = tail - w * 8 < 8 ? tail - w * 8 : 8;
            for (size_t b = 0; b < n; ++b) word |= (unsigned long long)p[done + w * 8 + b] << (8 * b);
            acc += mf::mix64(word ^ ((2 * pieces + w + 1) * K));
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ unsigned long long part[CHECKSUM_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < CHECKSUM_THREADS / 64; ++w) s += part[w];
        atomicAdd(sum, s);
    }
}

extern "C" int ivit_constants_checksum(ivit_handle h, const void *dev, size_t bytes, uint64_t *sum_dev) {
    CHECK_H(h);
    REQUIRE(h, sum_dev && (dev || bytes == 0), "sum_dev is null, or dev is null with bytes > 0");
    REQUIRE_A16(h, dev, "dev");
    REQUIRE_ALIGNED(h, sum_dev, "sum_dev", 8);
    REQUIRE_DISJOINT(h, dev, bytes, "dev", sum_dev, 8, "sum_dev", OVL_IN);
    hipError_t err = hipMemsetAsync(sum_dev, 0, 8, h->stream);
    if (err != hipSuccess) { snprintf(h->err, sizeof(h->err), "%s: %s", __func__, hipGetErrorString(err)); return IVIT_ERR_HIP; }
    if (bytes == 0) return IVIT_OK;
    // a thread works 16 bytes a step: enough workgroups for one step, capped at four per CU (the rest is the grid stride)
    const size_t want = (bytes / 16 + CHECKSUM_THREADS - 1) / CHECKSUM_THREADS;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(want, (size_t)4 * std::max(1, h->num_cu)));
    constants_checksum_kernel<<<grid, CHECKSUM_THREADS, 0, h->stream>>>((const uint8_t *)dev, bytes, (unsigned long long *)sum_dev);
    LAUNCH_CHECK(h);
    return IVIT_OK;
}

// ---- file -> live model
struct ivit_model_s {
    ivit_handle h = nullptr;
    int kind = 0;
    ivit_vit vit = nullptr;
    ivit_swin swin = nullptr;
    uint8_t *blob = nullptr;                 // the ONE device allocation
    ivit_model_info info;
    std::vector<char> names;                 // the record table, kept for ivit_model_constant: names, offsets, sizes
    struct Entry { size_t name, offset, bytes; };
    std::vector<Entry> entries;
};

static void model_free(ivit_model_s *m) {
    if (!m) return;
    if (m->vit) (void)ivit_vit_destroy(m->vit);
    if (m->swin) (void)ivit_swin_destroy(m->swin);
    if (m->blob) (void)hipFree(m->blob);
    delete m;
}

// upload `n` bytes through two pinned staging buffers on the handle's stream, then the device checksum against `want`
static int model_upload(ivit_handle h, const char *fn, const uint8_t *src, size_t n, uint8_t *dst, uint64_t want) {
    const size_t PIECE = (size_t)4 << 20;
    uint8_t *stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    uint64_t *sum_dev = nullptr;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipHostMalloc((void **)&stage[i], PIECE, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&sum_dev, 8);
    int rc = IVIT_OK;
    size_t off = 0;
    for (int i = 0; e == hipSuccess && off < n; ++i, off += PIECE) {
        const int s = i & 1;
        const size_t len = std::min(PIECE, n - off);
        if (i >= 2) e = hipEventSynchronize(done[s]);                 // the copy that read this staging buffer last has finished
        if (e != hipSuccess) break;
        memcpy(stage[s], src + off, len);
        e = hipMemcpyAsync(dst + off, stage[s], len, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipEventRecord(done[s], h->stream);
    }
    uint64_t got = 0;
    if (e == hipSuccess) rc = ivit_constants_checksum(h, dst, n, sum_dev);
    if (e == hipSuccess && rc == IVIT_OK) e = hipMemcpyAsync(&got, sum_dev, 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && rc == IVIT_OK) e = hipStreamSynchronize(h->stream);
    else (void)hipStreamSynchronize(h->stream);                        // nothing may still read the staging buffers
    for (int i = 0; i < 2; ++i) {
        if (done[i]) (void)hipEventDestroy(done[i]);
        if (stage[i]) (void)hipHostFree(stage[i]);
    }
    if (sum_dev) (void)hipFree(sum_dev);
    if (e != hipSuccess) { snprintf(h->err, sizeof(h->err), "%s: upload: %s", fn, hipGetErrorString(e)); return IVIT_ERR_HIP; }
    if (rc != IVIT_OK) return rc;
    if (got != want) {
        snprintf(h->err, sizeof(h->err), "%s: blob: device checksum %016llx, the file says %016llx", fn, (unsigned long long)got, (unsigned long long)want);
        return IVIT_ERR_HIP;
    }
    return IVIT_OK;
}

static int model_open_bytes(ivit_handle h, const char *fn, const uint8_t *data, size_t size, int max_slices, ivit_model *out) {
    mf::File f;
    mf::Err e;
    if (!mf::validate(data, size, &f, &e)) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, e.msg); return e.status; }
    if (max_slices < 1 || max_slices > 16) { snprintf(h->err, sizeof(h->err), "%s: max_slices must be in [1, 16]", fn); return IVIT_ERR_INVALID; }
    ivit_model_s *m = new (std::nothrow) ivit_model_s();
    if (!m) { snprintf(h->err, sizeof(h->err), "%s: out of host memory", fn); return IVIT_ERR_HIP; }
    m->h = h; m->kind = (int)f.kind;
    mf::info_of(f, &m->info);
    const hipError_t he = hipMalloc((void **)&m->blob, (size_t)f.blob_bytes);
    if (he != hipSuccess) {
        m->blob = nullptr;
        snprintf(h->err, sizeof(h->err), "%s: hipMalloc of %llu bytes: %s", fn, (unsigned long long)f.blob_bytes, hipGetErrorString(he));
        model_free(m);
        return IVIT_ERR_HIP;
    }
    int rc = model_upload(h, fn, f.blob(), (size_t)f.blob_bytes, m->blob, f.blob_sum);
    if (rc == IVIT_OK) {
        if (f.kind == mf::KIND_VIT) {
            ivit_vit_config c; ivit_vit_params p; std::vector<ivit_vit_block> b;
            if (!mf::fill_vit(f, (uintptr_t)m->blob, &c, &p, &b, &e)) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, e.msg); rc = e.status; }
            else rc = ivit_vit_create(h, &c, &p, max_slices, &m->vit);
        } else {
            ivit_swin_config c; ivit_swin_params p; std::vector<ivit_swin_block> b; std::vector<ivit_swin_merge> g;
            if (!mf::fill_swin(f, (uintptr_t)m->blob, &c, &p, &b, &g, &e)) { snprintf(h->err, sizeof(h->err), "%s: %s", fn, e.msg); rc = e.status; }
            else rc = ivit_swin_create(h, &c, &p, max_slices, &m->swin);
        }
    }
    if (rc != IVIT_OK) { model_free(m); return rc; }
    for (const mf::Rec &r : f.recs) {
        m->entries.push_back({m->names.size(), (size_t)r.offset, (size_t)r.bytes});
        m->names.insert(m->names.end(), r.name, r.name + strlen(r.name) + 1);
    }
    *out = m;
    return IVIT_OK;
}

extern "C" int ivit_model_open_memory(ivit_handle h, const void *file_bytes, size_t n, int max_slices, ivit_model *out) {
    if (out) *out = nullptr;
    CHECK_H(h);
    REQUIRE(h, file_bytes && out, "file_bytes or out is null");
    return model_open_bytes(h, __func__, (const uint8_t *)file_bytes, n, max_slices, out);
}

extern "C" int ivit_model_open(ivit_handle h, const char *path, int max_slices, ivit_model *out) {
    if (out) *out = nullptr;
    CHECK_H(h);
    REQUIRE(h, path && out, "path or out is null");
    std::vector<uint8_t> bytes;
    mf::Err e;
    if (!mf::read_file(path, &bytes, &e)) { snprintf(h->err, sizeof(h->err), "%s: %s", __func__, e.msg); return e.status; }
    return model_open_bytes(h, __func__, bytes.data(), bytes.size(), max_slices, out);
}

extern "C" int ivit_model_get_info(ivit_model m, ivit_model_info *info) {
    if (!m || !info) return IVIT_ERR_INVALID;
    *info = m->info;
    return IVIT_OK;
}

extern "C" int ivit_model_vit(ivit_model m, ivit_vit *out) {
    if (out) *out = nullptr;
    if (!m || !out || !m->vit) return IVIT_ERR_INVALID;
    *out = m->vit;
    return IVIT_OK;
}

extern "C" int ivit_model_swin(ivit_model m, ivit_swin *out) {
    if (out) *out = nullptr;
    if (!m || !out || !m->swin) return IVIT_ERR_INVALID;
    *out = m->swin;
    return IVIT_OK;
}

extern "C" int ivit_model_constant(ivit_model m, const char *name, const void **dev, size_t *bytes) {
    if (dev) *dev = nullptr;
    if (bytes) *bytes = 0;
    if (!m || !name) return IVIT_ERR_INVALID;
    for (const auto &en : m->entries) {
        if (strcmp(m->names.data() + en.name, name) == 0) {
            if (dev) *dev = m->blob + en.offset;
            if (bytes) *bytes = en.bytes;
            return IVIT_OK;
        }
    }
    snprintf(m->h->err, sizeof(m->h->err), "%s: the model holds no record \"%s\"", __func__, name);
    return IVIT_ERR_INVALID;
}

extern "C" int ivit_model_close(ivit_model m) {
    if (!m) return IVIT_ERR_INVALID;
    ivit_device_guard guard;
    if (!guard.enter(m->h->device)) return IVIT_ERR_HIP;
    model_free(m);
    return IVIT_OK;
}
#endif  // IVIT_MODELFILE_HOST_ONLY
