"""Frozen model files (include/ivit_modelfile.h, format version 1): everything a forward needs in one self-describing file — the
configuration, the packed constants blob with its record table, the host scalars — written once and read by the C library
(`ivit_model_open`) and by `ivit_amd.load_engine`.  The layout is stated once, in the header; this module is its numpy statement:

    write(path, kind, cfg, blob, table, scalars, extras) -> path
    read(path) -> (kind, cfg, blob, table, scalars, extras)          read_bytes(data) likewise
    freeze_to_file(cfg, weights, scales, path) -> path               float weights + scales -> file, host only
    checksum_reference(data) -> int                                  the 64-bit checksum of the header and of the blob
    load_engine(path, device="cuda:0") -> ViTEngine | SwinEngine     (needs a device; also `ivit_amd.load_engine`)

kind is "vit" or "swin"; cfg a ViTConfig / SwinConfig; (blob, table) what `engine.pack_constants` gives, every record at exactly its
offset; scalars name -> ("f", float32 value) | ("dy", m, r) | ("i", int32 value) — `ViTEngine.f32` as "f" entries, or the `host` dict
of `pack_swin_constants`, and "input.s", the scale of qact_input that the int8 images are quantised at; extras name -> array: records
that exist only for the file (a Swin's "class_scale"), appended behind the blob.  write / read / freeze_to_file are pure numpy: no
GPU, no library.  `read` validates what the C reader validates (csrc/ivit_modelfile.h), in the same order and with the same wording:
a ModelFileError carries `status` (IVIT_ERR_INVALID, or IVIT_ERR_UNSUPPORTED for a newer format or an unknown kind) and the text.
The bytes are deterministic: no time stamps, records and scalars sorted by name, padding zero."""
import struct

import numpy as np

from . import _abi
from .synth import SwinConfig, ViTConfig

FORMAT = 1
MAGIC = b"IVITMDL\0"
HEADER, RECORD, SCALAR, NAME = 256, 96, 72, 48
MAX_COUNT, MAX_DIM, MAX_DEPTH = 65536, 1 << 20, 4096
KINDS = {"vit": 1, "swin": 2}
DTYPES = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "f4", 7: "f8"}
DTYPE_CODES = {np.dtype(v).str: k for k, v in DTYPES.items()}
SCALAR_KINDS = {"f": 1, "dy": 2, "i": 3}
INVALID, UNSUPPORTED = _abi.ABI.constants["IVIT_ERR_INVALID"], _abi.ABI.constants["IVIT_ERR_UNSUPPORTED"]
_K = np.uint64(0x9E3779B97F4A7C15)


class ModelFileError(ValueError):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


def _fail(msg, status=INVALID):
    raise ModelFileError(status, msg)


def checksum_reference(data, skip=None):
    """the checksum of include/ivit_modelfile.h over bytes (bytes-like or a uint8 array): little-endian 64-bit words, the tail
    zero-padded; term i = mix(word_i ^ ((i + 1) * 0x9E3779B97F4A7C15)), mix the splitmix64 finaliser; the sum mod 2^64.  mix is a
    bijection, so any single changed word changes the sum, and the sum does not depend on the order of addition.  A zero byte appended
    inside the last word does not change the sum — harmless: the file stores every length.  `skip`: a byte offset (a multiple of 8)
    whose word is taken as 0, which is how the header's sum leaves out its own field."""
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    n = a.size
    if n % 8:
        a = np.concatenate([a, np.zeros(8 - n % 8, np.uint8)])
    w = a.view("<u8").astype(np.uint64)
    if skip is not None and skip // 8 < w.size:
        w = w.copy()
        w[skip // 8] = 0
    with np.errstate(over="ignore"):
        z = w ^ (np.arange(1, w.size + 1, dtype=np.uint64) * _K)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return int(z.sum(dtype=np.uint64))


def _cfg_fields(kind, cfg):
    """the fields of ivit_vit_config / ivit_swin_config in declaration order, padded to 16"""
    if kind == "vit":
        c = [cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.hidden_dim, cfg.num_classes]
        if cfg.hidden_dim != cfg.embed_dim * int(cfg.mlp_ratio):
            raise ValueError("hidden_dim must be a whole multiple of embed_dim")
    else:
        if len(cfg.depths) != len(cfg.num_heads) or not 1 <= len(cfg.depths) <= 4:
            raise ValueError("a Swin has 1 .. 4 stages")
        c = [cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim, cfg.num_layers, cfg.window_size, int(cfg.mlp_ratio), cfg.num_classes]
        c += (list(cfg.depths) + [0] * 4)[:4] + (list(cfg.num_heads) + [0] * 4)[:4]
    return [int(v) for v in c] + [0] * (16 - len(c))


def _cfg_from_fields(kind, c, name):
    if kind == "vit":
        return ViTConfig(name, img_size=c[0], patch_size=c[1], in_chans=c[2], num_classes=c[7], embed_dim=c[3], depth=c[4], num_heads=c[5],
                         mlp_ratio=c[6] // c[3])
    n = c[4]
    return SwinConfig(name, img_size=c[0], patch_size=c[1], in_chans=c[2], num_classes=c[7], embed_dim=c[3], depths=tuple(c[8:8 + n]),
                      num_heads=tuple(c[12:12 + n]), window_size=c[5], mlp_ratio=c[6])


def _name_field(name, what):
    b = name.encode("ascii")
    if not b or len(b) >= NAME or b"\0" in b:
        raise ValueError(f"{what} name {name!r}: 1 .. {NAME - 1} ASCII bytes")
    return b.ljust(NAME, b"\0")


def to_bytes(kind, cfg, blob, table, scalars, extras=None):
    """the file as bytes (what `write` writes)"""
    code = KINDS[kind]
    blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    core = blob.size
    if core % 256:
        raise ValueError("the blob is not a multiple of 256 bytes: not pack_constants' layout")
    records, tail, off = [], [], core
    for name, (o, dt, shp) in table.items():
        records.append((name, DTYPE_CODES[np.dtype(dt).str], tuple(int(d) for d in shp), int(o)))
    for name in sorted(extras or {}):
        a = np.ascontiguousarray(extras[name])
        if name in table:
            raise ValueError(f"extra record {name!r} is also in the table")
        records.append((name, DTYPE_CODES[a.dtype.str], a.shape, off))
        pad = -a.nbytes % 256
        tail += [a.view(np.uint8).reshape(-1), np.zeros(pad, np.uint8)]
        off += a.nbytes + pad
    whole = np.concatenate([blob] + tail) if tail else blob
    rec_bytes = b""
    for name, dt, shp, o in sorted(records):
        if not 1 <= len(shp) <= 3 or any(d < 1 for d in shp):
            raise ValueError(f"record {name!r}: shape {shp} (rank 1 .. 3, no empty dimension)")
        nbytes = int(np.prod(shp, dtype=np.int64)) * np.dtype(DTYPES[dt]).itemsize
        rec_bytes += _name_field(name, "record") + struct.pack("<II3QQQ", dt, len(shp), *(list(shp) + [0, 0, 0])[:3], o, nbytes)
    sca_bytes = b""
    for name in sorted(scalars):
        v = scalars[name]
        k = SCALAR_KINDS[v[0]]
        value = struct.pack("<f", v[1]) if k == 1 else struct.pack("<dd", v[1], v[2]) if k == 2 else struct.pack("<i", v[1])
        sca_bytes += _name_field(name, "scalar") + struct.pack("<II", k, 0) + value.ljust(16, b"\0")
    header_bytes = HEADER + len(rec_bytes) + len(sca_bytes)
    blob_offset = -(-header_bytes // 256) * 256
    cname = cfg.name.encode("ascii")
    if len(cname) >= 64:
        raise ValueError("configuration name: at most 63 bytes")
    fixed = MAGIC + struct.pack("<II5QII", FORMAT, code, blob_offset + whole.size, header_bytes, blob_offset, whole.size, core,
                                len(records), len(scalars))
    fixed += struct.pack("<QQ", 0, checksum_reference(whole)) + struct.pack("<16i", *_cfg_fields(kind, cfg)) + cname.ljust(64, b"\0")
    head = (fixed.ljust(HEADER, b"\0") + rec_bytes + sca_bytes).ljust(blob_offset, b"\0")
    head = head[:64] + struct.pack("<Q", checksum_reference(head, skip=64)) + head[72:]
    return head + whole.tobytes()


def write(path, kind, cfg, blob, table, scalars, extras=None):
    with open(path, "wb") as f:
        f.write(to_bytes(kind, cfg, blob, table, scalars, extras))
    return path


# ---------------------------------------------------------------- the reader: csrc/ivit_modelfile.h, check for check
def _check_config(kind, c):
    def rng(what, v, lo, hi):
        if not lo <= v <= hi:
            _fail(f"config: {what} {v} is outside {lo} .. {hi}")
    if kind == 1:
        rng("depth", c[4], 1, MAX_DEPTH)
        for what, v in zip(("img_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads", "hidden_dim", "num_classes"), c):
            rng(what, v, 1, MAX_DIM)
        for i in range(8, 16):
            if c[i]:
                _fail(f"config: unused field {i} is {c[i]}, not 0")
        if c[0] % c[1]:
            _fail(f"config: img_size {c[0]} is not a multiple of patch_size {c[1]}")
        if c[3] % c[5]:
            _fail(f"config: embed_dim {c[3]} is not a multiple of num_heads {c[5]}")
        if c[0] // c[1] > 1024:
            _fail(f"config: a grid of {c[0] // c[1]} patches a side is outside 1 .. 1024")
        return
    rng("num_layers", c[4], 1, 4)
    for i, what in enumerate(("img_size", "patch_size", "in_chans", "embed_dim", "num_layers", "window_size", "mlp_ratio", "num_classes")):
        rng(what, c[i], 1, 64 if i == 6 else MAX_DIM)
    rng("window_size", c[5], 1, 64)
    rng("embed_dim", c[3], 1, MAX_DIM >> 4)
    for li in range(4):
        if li < c[4]:
            rng("depth", c[8 + li], 1, MAX_DEPTH)
            rng("num_heads", c[12 + li], 1, 1024)
            if (c[3] << li) % c[12 + li]:
                _fail(f"config: stage {li}: width {c[3] << li} is not a multiple of num_heads {c[12 + li]}")
        elif c[8 + li] or c[12 + li]:
            _fail(f"config: stage {li} is beyond num_layers {c[4]} but has depth {c[8 + li]} and num_heads {c[12 + li]}")
    if c[0] % c[1]:
        _fail(f"config: img_size {c[0]} is not a multiple of patch_size {c[1]}")
    if (c[0] // c[1]) % (1 << (c[4] - 1)) or c[0] // c[1] > 4096:
        _fail(f"config: a grid of {c[0] // c[1]} patches a side does not halve {c[4] - 1} times")


def _terminated(field):
    i = field.find(b"\0")
    return None if i <= 0 else field[:i].decode("latin-1")


class _Fill:
    """the required-record check: the walk of mf::fill_vit / mf::fill_swin (the counterpart of vit_native_params /
    swin_native_params) without the structs"""

    def __init__(self, recs, scas, blob):
        self.recs, self.scas, self.blob = recs, scas, blob

    def rec(self, name, dt, *shape):
        r = self.recs.get(name)
        if r is None:
            _fail(f'model: record "{name}" is missing')
        have, want = (list(r[1]) + [0, 0, 0])[:3], (list(shape) + [0, 0, 0])[:3]
        if r[0] != dt or len(r[1]) != len(shape) or have != want:
            _fail(f'model: record "{name}" is {DTYPES[r[0]]} [{have[0]}, {have[1]}, {have[2]}], the configuration implies '
                  f'{DTYPES[dt]} [{want[0]}, {want[1]}, {want[2]}]')
        return r

    def scalar(self, name, kind):
        s = self.scas.get(name)
        if s is None:
            _fail(f'model: scalar "{name}" is missing')
        if SCALAR_KINDS[s[0]] != kind:
            _fail(f'model: scalar "{name}" has kind {SCALAR_KINDS[s[0]]}, not {kind}')
        return s

    def f32(self, name):
        return self.scalar(name, 1)[1]

    def dy(self, name):
        self.scalar(name, 2)

    def dy_blob(self, name):
        self.rec(name, 7, 1, 2)

    def ln(self, p, C):
        self.rec(p + ".bias_int", 6, C), self.rec(p + ".sc", 6, C), self.rec(p + ".dy", 7, C, 2)

    def lin(self, p, N, K, bias=True, dy=True):
        self.rec(p + ".w", 1, N, K)
        if bias:
            self.rec(p + ".b", 5, N)
        if dy:
            self.rec(p + ".dy", 7, N, 2)

    def exp_tables(self, p, nc, tcount, dmin):
        if nc < 1 or nc > 256 or tcount < 1 or tcount > 65535 or dmin > 0 or dmin < -255:
            _fail(f'model: Shiftmax tables of "{p}attn": metadata ({nc}, {tcount}, {dmin}) is out of range')
        self.rec(p + "attn.exp_aq", 4, nc, 256), self.rec(p + "attn.exp_t", 6, tcount), self.rec(p + "attn.exp_cls", 2, 256)


def _check_vit(c, F):
    D, Hd, NC, g = c[3], c[6], c[7], c[0] // c[1]
    T, Kp = g * g + 1, c[2] * c[1] * c[1]
    for i in range(c[4]):
        p = f"blocks.{i}."
        F.f32(p + "ln1.s"), F.ln(p + "norm1", D), F.lin(p + "attn.qkv", 3 * D, D)
        F.dy_blob(p + "attn.dy_qk"), F.f32(p + "attn.s_softmax"), F.dy_blob(p + "attn.dy_pv")
        have = sum(p + n in F.recs for n in ("attn.exp_meta", "attn.exp_aq", "attn.exp_t", "attn.exp_cls"))
        if have not in (0, 4):
            _fail(f'model: Shiftmax tables of "{p}attn" are partly present ({have} of 4 records)')
        if have == 4:
            o = F.rec(p + "attn.exp_meta", 5, 3)[2]
            meta = F.blob[o:o + 12].view("<i4")
            F.exp_tables(p, int(meta[0]), int(meta[1]), int(meta[2]))
        F.lin(p + "attn.proj", D, D), F.dy_blob(p + "res1.dy_main"), F.dy_blob(p + "res1.dy_res")
        F.f32(p + "ln2.s"), F.ln(p + "norm2", D), F.lin(p + "mlp.fc1", Hd, D), F.f32(p + "mlp.s_gelu"), F.dy_blob(p + "mlp.dy_gelu")
        F.lin(p + "mlp.fc2", D, Hd), F.dy_blob(p + "res2.dy_main"), F.dy_blob(p + "res2.dy_res")
    F.lin("patch_embed.proj", D, Kp), F.rec("z_cls", 5, D), F.rec("pos", 3, T, D), F.dy_blob("embed.dy_x"), F.dy_blob("embed.dy_pos")
    F.f32("ln.s"), F.ln("norm", D), F.lin("head", NC, D, dy=False), F.rec("head.scale", 6, NC), F.f32("input.s"), F.f32("feat.s")


def _check_swin(c, F):
    E, L, NC, R, grid = c[3], c[4], c[7], c[6], c[0] // c[1]
    Kp = c[2] * c[1] * c[1]
    for li in range(L):
        C, heads, res = E << li, c[12 + li], grid >> li
        N = min(c[5], res) ** 2
        for bj in range(c[8 + li]):
            p = f"layers.{li}.blocks.{bj}."
            F.f32(p + "s_in"), F.ln(p + "norm1", C), F.lin(p + "attn.qkv", 3 * C, C), F.dy(p + "attn.dy_qk"), F.dy(p + "attn.dy_a")
            F.rec(p + "attn.relb", 3, heads, N, N), F.f32(p + "attn.s_softmax"), F.dy(p + "attn.dy_pv"), F.lin(p + "attn.proj", C, C)
            have = sum(p + n in F.recs for n in ("attn.exp_aq", "attn.exp_t", "attn.exp_cls"))
            meta = sum(p + n in F.scas for n in ("attn.exp_nc", "attn.exp_tcount", "attn.exp_dmin"))
            if have not in (0, 3) or meta != have:
                _fail(f'model: Shiftmax tables of "{p}attn" are partly present ({have} of 3 records, {meta} of 3 scalars)')
            if have == 3:
                m = [F.f32(p + n) for n in ("attn.exp_nc", "attn.exp_tcount", "attn.exp_dmin")]
                sane = 0 <= m[0] <= 65536 and 0 <= m[1] <= 65536 and -65536 <= m[2] <= 65536
                F.exp_tables(p, *((int(m[0]), int(m[1]), int(m[2])) if sane else (-1, -1, 1)))
            F.dy(p + "res1.dy_main"), F.dy(p + "res1.dy_res"), F.f32(p + "s_mid"), F.ln(p + "norm2", C), F.lin(p + "mlp.fc1", R * C, C)
            F.f32(p + "mlp.s_gelu"), F.dy(p + "mlp.dy_gelu"), F.lin(p + "mlp.fc2", C, R * C), F.dy(p + "res2.dy_main"), F.dy(p + "res2.dy_res")
        if li < L - 1:
            p = f"layers.{li}.downsample."
            F.f32(p + "s_in"), F.ln(p + "norm", 4 * C), F.lin(p + "reduction", 2 * C, 4 * C, bias=False)
    CL = E << (L - 1)
    F.lin("patch_embed.proj", E, Kp), F.f32("patch_embed.s_bn"), F.ln("patch_embed.norm", E), F.rec("dy_qact1", 7, 1, 2)
    F.f32("norm.s_in"), F.ln("norm", CL), F.dy("dy_pool"), F.lin("head", NC, CL, dy=False), F.f32("pool.s_in")
    F.rec("head.scale", 6, NC), F.rec("class_scale", 6, NC), F.f32("input.s"), F.f32("feat.s")


def read_bytes(data):
    """the bytes of a file -> (kind, cfg, blob, table, scalars, extras); ModelFileError with the C reader's status and text"""
    data = bytes(data)
    size = len(data)
    if size < HEADER:
        _fail(f"header: file holds {size} bytes, fewer than the {HEADER} of the fixed header")
    if data[:8] != MAGIC:
        _fail("header: bad magic")
    fmt, code, file_bytes, header_bytes, blob_offset, blob_bytes, core, nrec, nsca, hsum, bsum = struct.unpack_from("<II5QIIQQ", data, 8)
    if fmt == 0:
        _fail("header: format version 0")
    if fmt > FORMAT:
        _fail(f"header: format version {fmt} is newer than 1", UNSUPPORTED)
    if code not in (1, 2):
        _fail(f"header: unknown kind {code}", UNSUPPORTED)
    if file_bytes != size:
        _fail(f"header: file holds {size} bytes, its header says {file_bytes}")
    if blob_offset < HEADER or blob_offset > size or blob_offset % 256:
        _fail(f"header: blob offset {blob_offset} is not a multiple of 256 inside the file of {size} bytes")
    if blob_bytes != size - blob_offset:
        _fail(f"header: blob of {blob_bytes} bytes at offset {blob_offset} does not end with the file of {size} bytes")
    if core > blob_bytes or core % 256:
        _fail(f"header: core size {core} is not a multiple of 256 within the blob of {blob_bytes} bytes")
    got = checksum_reference(data[:blob_offset], skip=64)
    if got != hsum:
        _fail(f"header: checksum {got:016x}, the header says {hsum:016x}")
    if nrec > MAX_COUNT:
        _fail(f"records: count {nrec} exceeds {MAX_COUNT}")
    if nsca > MAX_COUNT:
        _fail(f"scalars: count {nsca} exceeds {MAX_COUNT}")
    tables_end = HEADER + RECORD * nrec + SCALAR * nsca
    if header_bytes != tables_end or blob_offset != -(-tables_end // 256) * 256:
        _fail(f"header: tables of {nrec} records and {nsca} scalars end at {tables_end}, the header says {header_bytes} and the blob starts "
              f"at {blob_offset}")
    for i in range(208, HEADER):
        if data[i]:
            _fail(f"header: reserved byte {i} is not 0")
    for i in range(tables_end, blob_offset):
        if data[i]:
            _fail(f"header: padding byte {i} is not 0")
    c = list(struct.unpack_from("<16i", data, 80))
    if b"\0" not in data[144:208]:
        _fail("config: name is not terminated")
    cname = data[144:208].split(b"\0")[0].decode("latin-1")
    _check_config(code, c)

    recs, prev = {}, None
    for i in range(nrec):
        p = HEADER + RECORD * i
        name = _terminated(data[p:p + NAME])
        if name is None:
            _fail(f"records: record {i}: name is empty or not terminated")
        dt, rank, s0, s1, s2, off, nbytes = struct.unpack_from("<II3QQQ", data, p + NAME)
        if prev is not None and prev == name:
            _fail(f'records: record {i} "{name}": duplicate name')
        if prev is not None and prev.encode("latin-1") > name.encode("latin-1"):
            _fail(f'records: record {i} "{name}": names are not sorted')
        prev = name
        if not 1 <= dt <= 7:
            _fail(f'records: record {i} "{name}": unknown dtype code {dt}')
        if not 1 <= rank <= 3:
            _fail(f'records: record {i} "{name}": rank {rank} is outside 1 .. 3')
        want = np.dtype(DTYPES[dt]).itemsize
        for d, s in enumerate((s0, s1, s2)):
            if d >= rank:
                if s:
                    _fail(f'records: record {i} "{name}": unused dimension {d} is {s}, not 0')
                continue
            if s < 1 or s > 1 << 32 or want > (1 << 62) // s:
                _fail(f'records: record {i} "{name}": dimension {d} is {s}')
            want *= s
        if nbytes != want:
            _fail(f'records: record {i} "{name}": {nbytes} bytes, its shape and dtype give {want}')
        if off % 256:
            _fail(f'records: record {i} "{name}": offset {off} is not a multiple of 256')
        if nbytes > blob_bytes or off > blob_bytes - nbytes:
            _fail(f'records: record {i} "{name}": offset {off} + {nbytes} bytes passes the blob of {blob_bytes}')
        if off < core < off + nbytes:
            _fail(f'records: record {i} "{name}": offset {off} + {nbytes} bytes crosses the core size {core}')
        recs[name] = (dt, (s0, s1, s2)[:rank], off, nbytes)
    order = [n for _, _, n in sorted((recs[n][2], i, n) for i, n in enumerate(recs))]       # overlaps: by offset
    for a, b in zip(order, order[1:]):
        if recs[a][2] + recs[a][3] > recs[b][2]:
            _fail(f'records: records "{a}" and "{b}" overlap at offset {recs[b][2]}')
    scas, prev = {}, None
    for i in range(nsca):
        p = HEADER + RECORD * nrec + SCALAR * i
        name = _terminated(data[p:p + NAME])
        if name is None:
            _fail(f"scalars: scalar {i}: name is empty or not terminated")
        k = struct.unpack_from("<I", data, p + NAME)[0]
        if prev is not None and prev == name:
            _fail(f'scalars: scalar {i} "{name}": duplicate name')
        if prev is not None and prev.encode("latin-1") > name.encode("latin-1"):
            _fail(f'scalars: scalar {i} "{name}": names are not sorted')
        prev = name
        if not 1 <= k <= 3:
            _fail(f'scalars: scalar {i} "{name}": unknown kind {k}')
        used = 16 if k == 2 else 4
        for b in range(52, SCALAR):
            if (b < 56 or b >= 56 + used) and data[p + b]:
                _fail(f'scalars: scalar {i} "{name}": unused byte {b} is not 0')
        if k == 1:
            scas[name] = ("f", float(np.frombuffer(data, "<f4", 1, p + 56)[0]))
        elif k == 2:
            scas[name] = ("dy",) + struct.unpack_from("<dd", data, p + 56)
        else:
            scas[name] = ("i", struct.unpack_from("<i", data, p + 56)[0])
    whole = np.frombuffer(data, np.uint8, blob_bytes, blob_offset)
    got = checksum_reference(whole)
    if got != bsum:
        _fail(f"blob: checksum {got:016x}, the header says {bsum:016x}")
    (_check_vit if code == 1 else _check_swin)(c, _Fill(recs, scas, whole))

    kind = "vit" if code == 1 else "swin"
    table, extras = {}, {}
    for name, (dt, shp, off, nbytes) in recs.items():
        dtype = np.dtype(DTYPES[dt])
        if off < core:
            table[name] = (off, dtype.str, tuple(shp))
        else:
            extras[name] = whole[off:off + nbytes].view(dtype).reshape(shp).copy()
    return kind, _cfg_from_fields(kind, c, cname), whole[:core].copy(), table, scas, extras


def read(path):
    """file -> (kind, cfg, blob, table, scalars, extras), validated as the C reader validates it"""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        _fail(f'file: cannot open "{path}"')
    return read_bytes(data)


# ---------------------------------------------------------------- freezing and the engines
def frozen_package(cfg, weights, scales):
    """float weights + scales -> the arguments of `write` behind the path, through frozen_vit / packed_swin; host only"""
    from .freeze import quantize_weight
    s_in = float(np.float32(scales["qact_input"]))
    if isinstance(cfg, SwinConfig):
        from .swin_engine import packed_swin
        blob, table, host = packed_swin(cfg, weights, scales)
        fc_sf = quantize_weight(weights["head.weight"])[1]
        class_scale = (np.float32(host["pool.s_in"][1]) * fc_sf).astype(np.float32)     # SwinEngine.class_scale
        return "swin", cfg, blob, table, dict(host, **{"input.s": ("f", s_in)}), {"class_scale": class_scale}
    from .engine import frozen_vit, pack_constants
    consts, f32 = frozen_vit(cfg, weights, scales)
    blob, table = pack_constants(consts)
    scalars = {k: ("f", float(np.float32(v))) for k, v in f32.items()}
    return "vit", cfg, blob, table, dict(scalars, **{"input.s": ("f", s_in)}), {}


def freeze_to_file(cfg, weights, scales, path):
    """float weights + scales -> file; no device, no library"""
    return write(path, *frozen_package(cfg, weights, scales))


def load_engine(path, device="cuda:0"):
    """file -> ViTEngine / SwinEngine, through the constructors' pre-packed routes (blob= / table= of a ViT, packed= of a Swin); the
    engine behaves as the one that was saved, `input_scale_host()` and a Swin's `class_scale` included"""
    kind, cfg, blob, table, scalars, extras = read(path)
    s_in = scalars["input.s"][1]
    rest = {k: v for k, v in scalars.items() if k != "input.s"}
    if kind == "vit":
        from .engine import ViTEngine
        return ViTEngine(cfg, None, {k: v[1] for k, v in rest.items()}, device=device, blob=blob, table=table, input_scale=s_in)
    from .swin_engine import SwinEngine
    return SwinEngine(cfg, None, None, device=device, packed=(blob, table, rest), input_scale=s_in, class_scale=extras["class_scale"])
