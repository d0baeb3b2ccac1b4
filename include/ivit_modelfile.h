/*
 * ivit_modelfile.h — frozen model files: a model saved once (ivit_amd.model_file, engine.save, tools/freeze.py) and run from C with
 * no Python in the process.  ivit_model_open turns a file into a live ivit_vit / ivit_swin that every runner entry of the seven older
 * headers takes: forward, predict, score, features, attention, class_map, hidden_states, and ivit_search_* behind features.  Eighth
 * public header of libivit_hip.so.
 *
 * Why an eighth header: ivit.h is frozen at IVIT_VERSION 111, ivit_eval.h, ivit_features.h, ivit_attnmap.h, ivit_classmap.h,
 * ivit_hidden.h and ivit_search.h at their versions 1 (their prototypes and versions are pinned by the binding's tests), so these
 * entries are declared here, under a version of their own.  This header includes ivit.h and uses its handles (ivit_handle, ivit_vit,
 * ivit_swin) and its status codes.  Only those codes exist: an unreadable, truncated or malformed file is IVIT_ERR_INVALID, a newer
 * format version or an unknown kind IVIT_ERR_UNSUPPORTED; the text — it names the section, the record and the offending number — is in
 * `msg` (ivit_model_file_info) or ivit_last_error(h).
 *
 * ---- The file, format version 1.  Little-endian, fixed-width fields, no padding but what is stated; every byte not described is 0.
 *
 *   offset  field
 *        0  char     magic[8]        "IVITMDL\0"
 *        8  uint32   format          1
 *       12  uint32   kind            1 = ViT / DeiT (ivit_vit_config), 2 = Swin (ivit_swin_config)
 *       16  uint64   file_bytes      the whole file
 *       24  uint64   header_bytes    256 + 96 * records + 72 * scalars: the end of the scalar table
 *       32  uint64   blob_offset     header_bytes rounded up to a multiple of 256
 *       40  uint64   blob_bytes      file_bytes - blob_offset
 *       48  uint64   core_bytes      the blob as the engines' packer lays it out (ivit_amd.engine.pack_constants); records that exist
 *                                    only for the file (a Swin's "class_scale") lie behind it.  A multiple of 256, <= blob_bytes
 *       56  uint32   records, 60 uint32 scalars      table lengths, each <= 65536
 *       64  uint64   header_sum      the checksum below over bytes [0, blob_offset) with this field taken as 0
 *       72  uint64   blob_sum        the checksum below over the blob
 *       80  int32    config[16]      the fields of ivit_vit_config (8, the rest 0) or of ivit_swin_config (8, depths[4], num_heads[4]) in
 *                                    declaration order
 *      144  char     config_name[64] NUL-terminated ("deit_tiny")
 *      208  48 bytes reserved, 0
 *      256  record table, sorted by name (bytewise), 96 bytes each:
 *           char name[48] (NUL-terminated); uint32 dtype; uint32 rank (1 .. 3); uint64 shape[3] (unused: 0); uint64 offset (into the
 *           blob, a multiple of 256, exactly the packer's); uint64 bytes (the product of the shape times the item size)
 *           dtype codes: 1 int8, 2 uint8, 3 int16, 4 uint16, 5 int32, 6 float32, 7 float64
 *      then scalar table, sorted by name, 72 bytes each:
 *           char name[48]; uint32 kind; uint32 0; 16 bytes of value: kind 1 = one float32, kind 2 = a dyadic as two float64 (m, r),
 *           kind 3 = one int32; the rest 0.  "input.s" is the scale the int8 images are quantised at, "feat.s" that of the features
 *      then zeros up to blob_offset, then the blob.
 *
 *   The checksum of n bytes: split them into little-endian 64-bit words, the tail zero-padded; term i (from 0) is
 *   mix(word_i XOR ((i + 1) * 0x9E3779B97F4A7C15)) with mix the splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *   z *= 0x94D049BB133111EB; z ^= z >> 31); the checksum is the sum of the terms mod 2^64.  mix is a bijection, so changing any single
 *   word changes the sum; the sum does not depend on the order of addition, so a parallel reduction is exact.
 *   ivit_amd.model_file.checksum_reference is the numpy statement; the host reader and ivit_constants_checksum equal it bit for bit.
 *
 *   Deterministic: no time stamps, no host names; the same frozen model gives the same bytes.
 *
 * Deliberately not here: compression, encryption or signing; memory-mapped zero-copy; a file form of galleries; cross-version
 * migration (there is one version).
 */
#ifndef IVIT_MODELFILE_H
#define IVIT_MODELFILE_H

#include "ivit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: ivit_model_file_info, ivit_model_open, ivit_model_open_memory, ivit_model_get_info, ivit_model_vit, ivit_model_swin,
 * ivit_model_constant, ivit_model_close, ivit_constants_checksum. */
#define IVIT_MODELFILE_VERSION 1

typedef struct ivit_model_s *ivit_model;

/* ints, int64_t and floats only */
typedef struct ivit_model_info {
    int format, kind, img_size, in_chans, num_classes, num_features, records, scalars;
    int64_t file_bytes, blob_bytes;
    float s_input, s_features;
} ivit_model_info;

/* ---- m1  HOST ONLY, no handle, no device: opens and validates the WHOLE file — structure, both checksums, and every record and
 * scalar the model's parameter structs are filled from, with the dtype and shape the configuration implies — and reports what it
 * holds.  msg (may be NULL) receives the problem as a NUL-terminated text of at most msg_bytes bytes, "" on success.  A null path or
 * info is IVIT_ERR_INVALID.                                                                                                       */
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_file_info(const char *path, ivit_model_info *info, char *msg, size_t msg_bytes);

/* ---- m2  file -> live model: read and validate as m1, ONE device allocation for the blob, upload in pieces through pinned staging
 * on the handle's stream, ivit_constants_checksum of the device copy compared with the file's blob checksum, the parameter structs
 * filled with blob + offset (the name -> field mapping of ivit_amd.engine.vit_native_params / swin_engine.swin_native_params), then
 * ivit_vit_create / ivit_swin_create with max_slices.  Allocates and SYNCHRONISES, like every *_create.  On every error *out is NULL
 * and whatever was allocated is freed.  The handle must outlive the model.                                                         */
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_open(ivit_handle h, const char *path, int max_slices, ivit_model *out);

/* ---- m3  the same from the file's bytes in host memory (n of them); the bytes are not needed after the call.                    */
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_open_memory(ivit_handle h, const void *file_bytes, size_t n, int max_slices, ivit_model *out);

/* ---- m4  what m1 reports, of an open model.                                                                                    */
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_get_info(ivit_model m, ivit_model_info *info);

/* ---- m5, m6  the runner, BORROWED: it lives until ivit_model_close and every ivit_vit_* / ivit_swin_* entry of all seven headers
 * takes it.  IVIT_ERR_INVALID on the other kind (and *out NULL).                                                                 */
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_vit(ivit_model m, ivit_vit *out);
/* Alignment: none (host pointers). */
/* Overlap: none. */
int ivit_model_swin(ivit_model m, ivit_swin *out);

/* ---- m7  a record by name: *dev its DEVICE address inside the model's blob, *bytes its size (either may be NULL).  "head.scale"
 * (float [num_classes], what ivit_*_predict / _score take), a Swin's "class_scale" (float [num_classes], what ivit_swin_class_map
 * takes), any other record of the table.  An unknown name is IVIT_ERR_INVALID.                                                    */
/* Alignment: none (host pointers).  Every record's device address is 256-byte aligned. */
/* Overlap: none. */
int ivit_model_constant(ivit_model m, const char *name, const void **dev, size_t *bytes);

/* ---- m8  destroys the runner and frees the blob.                                                                               */
/* Alignment: none. */
/* Overlap: none. */
int ivit_model_close(ivit_model m);

/* ---- m9  the checksum above over `bytes` bytes of DEVICE memory, result in *sum_dev (device).  Asynchronous on the handle's stream,
 * nothing allocated, nothing synchronised, hipGraph-capturable: one 8-byte memset and one launch (csrc/ivit_modelfile.h) — a
 * grid-stride pass over 16-byte pieces, the tail read byte by byte and never beyond `bytes`, one atomic add per workgroup.  bytes
 * may be 0 (the sum is 0; dev may then be NULL) and may exceed 4 GiB.  What verifies a blob after ivit_constants_upload or
 * ivit_constants_broadcast.  A null sum_dev, or a null dev with bytes > 0, is IVIT_ERR_INVALID.                                  */
/* Alignment: dev 16-byte aligned, sum_dev 8-byte: IVIT_ERR_INVALID otherwise, nothing launched. */
/* Overlap: sum_dev may not overlap dev: IVIT_ERR_INVALID, nothing launched. */
int ivit_constants_checksum(ivit_handle h, const void *dev, size_t bytes, uint64_t *sum_dev);

#ifdef __cplusplus
}
#endif
#endif /* IVIT_MODELFILE_H */
