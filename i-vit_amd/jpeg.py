"""JPEG input (include/ivit_jpeg.h): the entropy decode on the host, everything behind the coefficients in one device call over a
ragged batch, into the pixel pool the eval transform and the views read.  The result is PIL's `Image.open(f).convert("RGB")`, every
byte, or the file is refused.

    jpeg_coefficients_reference(data)   the host half as numpy: parser and Huffman decode -> (JpegInfo, [int16 [blocks, 64]] per
                                        component); what csrc/ivit_jpeg_host.h computes, refusals included (JpegRefused)
    jpeg_reference(data)                both halves: uint8 [h, w, 3]; what the device call writes
    query / entropy_decode              the two host entries of the library (no GPU call)
    reconstruct                         the device entry on a batch of decoded files
    decode                              files or bytes -> (RaggedImages, fallbacks)

The definition is libjpeg's, with its defaults ("JPEG input", states it line by line): dequantise, the "islow" inverse DCT
(13-bit constants, a column pass to 2 extra bits, a row pass, +128, the range limit), "fancy" h2v1 / h2v2 chroma upsampling where the
subsampled plane is wider than two samples and replication where it is not, YCbCr -> RGB in 16-bit fixed point."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

IVIT_OK, IVIT_ERR_INVALID, IVIT_ERR_UNSUPPORTED = _lib.IVIT_OK, _lib.IVIT_ERR_INVALID, _lib.IVIT_ERR_UNSUPPORTED

# the host's bound (csrc/ivit_jpeg_host.h): the absolute values of the dequantised coefficients of every COLUMN of a block sum to at
# most this.  8-bit samples give at most 8 * 1024 / sqrt(8) = 2897 (+ the quantiser's rounding); below it every intermediate of
# the islow IDCT fits 16 bits after the column pass and 24 bits as a multiplicand, so the 16-bit SIMD forms of libjpeg-turbo and its
# C form compute the same samples.
COLUMN_BOUND = 2950
# ... and every sample before the range limit lies in [-512, 511], where the range limit's wrap-around and a saturation agree; checked
# exactly where the |.| of a whole block sum to more than SUM_EXACT (below it no sample can leave that range)
SUM_EXACT = 2040

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63], np.int32)          # zigzag position -> natural (row-major) position

JPEG_DESC_FIELDS = ("coef_offset", "pixel_offset", "plane_offset", "w", "h", "ncomp", "hs", "vs", "bw", "bh", "reserved", "qt")


class JpegRefused(ValueError):
    """a stream the decoder does not take: .status is IVIT_ERR_UNSUPPORTED or IVIT_ERR_INVALID, the text the reason"""
    def __init__(self, status, reason):
        super().__init__(reason)
        self.status, self.reason = status, reason


def _unsupported(msg):
    return JpegRefused(IVIT_ERR_UNSUPPORTED, msg)


def _invalid(msg):
    return JpegRefused(IVIT_ERR_INVALID, msg)


class JpegInfo:
    """what the parser knows at the start of the scan: w, h, ncomp, (hs, vs) the luma sampling, bw / bh the MCU-padded block grid of
    every component, qt uint8 [ncomp, 64] in natural order"""
    def __init__(self, w, h, ncomp, hs, vs, qt):
        self.w, self.h, self.ncomp, self.hs, self.vs = w, h, ncomp, hs, vs
        mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
        self.mcus = (mw, mh)
        self.bw = [mw * hs] + [mw] * (ncomp - 1)
        self.bh = [mh * vs] + [mh] * (ncomp - 1)
        self.qt = qt

    @property
    def blocks(self):
        return [a * b for a, b in zip(self.bw, self.bh)]


# ---------------------------------------------------------------- the host half, as numpy
class _Huff:
    def __init__(self, counts, values, dc):
        if sum(counts) > 256 or sum(counts) != len(values):
            raise _invalid("bad Huffman table")
        if dc and any(v > 15 for v in values):
            raise _invalid("bad Huffman table: DC category above 15")
        self.lookup = {}
        code = 0
        k = 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                if code >= (1 << length):
                    raise _invalid("bad Huffman table: code lengths overflow")
                self.lookup[(length, code)] = values[k]
                k += 1
                code += 1
            code <<= 1


class _Bits:
    """libjpeg's reading of entropy-coded bytes: FF 00 is a data FF, FF FF .. FF 00 too, FF x a marker, which ends the data"""
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.cnt, self.marker = data, pos, 0, 0, None

    def _byte(self):
        if self.marker is not None:
            raise _invalid("data ends before the last MCU")
        if self.p >= len(self.d):
            raise _invalid("data ends before the last MCU")
        c = self.d[self.p]
        self.p += 1
        if c == 0xFF:
            while True:
                if self.p >= len(self.d):
                    raise _invalid("data ends before the last MCU")
                c = self.d[self.p]
                self.p += 1
                if c != 0xFF:
                    break
            if c != 0:
                self.marker = c
                raise _invalid("data ends before the last MCU")
            c = 0xFF
        return c

    def bit(self):
        if self.cnt == 0:
            self.acc, self.cnt = self._byte(), 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, tbl):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = tbl.lookup.get((length, code))
            if s is not None:
                return s
        raise _invalid("Huffman code not in the table")

    def next_marker(self):
        """the marker behind the entropy-coded segment: the bits of the current byte are padding, no whole byte may be left"""
        if self.marker is not None:
            m, self.marker = self.marker, None
        else:
            if self.p + 1 >= len(self.d) or self.d[self.p] != 0xFF:
                raise _invalid("data ends before the last MCU" if self.p + 1 >= len(self.d) else "extraneous bytes before a marker")
            while self.p < len(self.d) and self.d[self.p] == 0xFF:
                self.p += 1
            if self.p >= len(self.d):
                raise _invalid("data ends before the last MCU")
            m = self.d[self.p]
            self.p += 1
            if m == 0:
                raise _invalid("extraneous bytes before a marker")
        self.acc = self.cnt = 0
        return m


def _extend(v, s):
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _parse(data):
    """-> (JpegInfo, scan components [(dc table, ac table)], restart interval, position of the entropy-coded bytes)"""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise _invalid("no SOI marker")
    pos = 2
    qt, dc, ac = [None] * 4, [None] * 4, [None] * 4
    frame, jfif, adobe, ri = None, False, None, 0
    while True:
        if pos >= n:
            raise _invalid("stream ends inside the headers")
        if d[pos] != 0xFF:
            raise _invalid("marker expected")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise _invalid("stream ends inside the headers")
        m = d[pos]
        pos += 1
        if m == 0xD9:
            raise _invalid("EOI before the image data")
        if m == 0x00 or m == 0x01 or m == 0xD8 or 0xD0 <= m <= 0xD7:
            raise _invalid("marker 0x%02X where a segment is expected" % m)
        if pos + 2 > n:
            raise _invalid("stream ends inside the headers")
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2 or pos + L > n:
            raise _invalid("bad segment length")
        seg = d[pos + 2:pos + L]
        pos += L
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise _invalid("two SOF markers")
            if len(seg) < 6:
                raise _invalid("bad SOF length")
            if seg[0] != 8:
                raise _unsupported("%d-bit samples (8-bit only)" % seg[0])
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc:
                raise _invalid("bad SOF length")
            if h == 0 or w == 0:
                raise _invalid("empty image")
            if nc == 4:
                raise _unsupported("4 components (CMYK / YCCK)")
            if nc not in (1, 3):
                raise _unsupported("%d components" % nc)
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            for cid, ch, cv, tq in comps:
                if not (1 <= ch <= 4 and 1 <= cv <= 4) or tq > 3:
                    raise _invalid("bad component in SOF")
            if len(set(c[0] for c in comps)) != nc:
                raise _invalid("duplicate component id")
            frame = (w, h, comps)
        elif m == 0xC2:
            raise _unsupported("progressive JPEG (SOF2)")
        elif m in (0xC3, 0xC7, 0xCB, 0xCF):
            raise _unsupported("lossless JPEG")
        elif m in (0xC9, 0xCA, 0xCD, 0xCE, 0xCC):
            raise _unsupported("arithmetic coding")
        elif m in (0xC5, 0xC6, 0xC8):
            raise _unsupported("hierarchical JPEG")
        elif m == 0xDC:
            raise _unsupported("DNL marker")
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if tq > 3 or pq > 1:
                    raise _invalid("bad DQT")
                if pq == 1:
                    raise _unsupported("16-bit quantisation table")
                if i + 65 > len(seg):
                    raise _invalid("bad DQT length")
                t = np.zeros(64, np.uint8)
                t[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                qt[tq] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise _invalid("bad DHT length")
                tc, th = seg[i] >> 4, seg[i] & 15
                if tc > 1 or th > 3:
                    raise _invalid("bad DHT")
                counts = list(seg[i + 1:i + 17])
                if sum(counts) > 256 or i + 17 + sum(counts) > len(seg):
                    raise _invalid("bad DHT length")
                tbl = _Huff(counts, list(seg[i + 17:i + 17 + sum(counts)]), tc == 0)
                (dc if tc == 0 else ac)[th] = tbl
                i += 17 + sum(counts)
        elif m == 0xDD:
            if len(seg) != 2:
                raise _invalid("bad DRI length")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            if len(seg) >= 14 and seg[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDA:
            if frame is None:
                raise _invalid("SOS before SOF")
            w, h, comps = frame
            nc = len(comps)
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise _invalid("bad SOS length")
            if seg[0] != nc:
                raise _unsupported("a scan of %d of %d components (one interleaved scan only)" % (seg[0], nc))
            tabs = []
            for i in range(nc):
                if seg[1 + 2 * i] != comps[i][0]:
                    raise _invalid("scan component out of order")
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if td > 3 or ta > 3:
                    raise _invalid("bad table selector in SOS")
                if dc[td] is None or ac[ta] is None:
                    raise _invalid("missing Huffman table")
                tabs.append((dc[td], ac[ta]))
            if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
                raise _invalid("spectral selection in a sequential scan")
            if nc == 3:
                if not jfif:
                    if adobe is not None:
                        if adobe == 0:
                            raise _unsupported("RGB-coded file (Adobe transform 0)")
                        if adobe != 1:
                            raise _unsupported("Adobe transform %d" % adobe)
                    elif tuple(c[0] for c in comps) == (0x52, 0x47, 0x42):
                        raise _unsupported("RGB-coded file (component ids R, G, B)")
                if (comps[1][1], comps[1][2], comps[2][1], comps[2][2]) != (1, 1, 1, 1) or (comps[0][1], comps[0][2]) not in (
                        (1, 1), (2, 1), (2, 2)):
                    raise _unsupported("sampling factors %s (4:4:4, 4:2:2 and 4:2:0 only)" % "/".join("%dx%d" % (c[1], c[2]) for c in comps))
                hs, vs = comps[0][1], comps[0][2]
            else:
                hs = vs = 1
            for c in comps:
                if qt[c[3]] is None:
                    raise _invalid("missing quantisation table")
            info = JpegInfo(w, h, nc, hs, vs, np.stack([qt[c[3]] for c in comps]))
            return info, tabs, ri, pos
        else:
            raise _invalid("unknown marker 0x%02X" % m)


def jpeg_coefficients_reference(data):
    """bytes -> (JpegInfo, [int16 [bw * bh, 64]] per component): the quantised coefficients in natural order, block-row-major over the
    component's MCU-padded grid, DC prediction undone.  Raises JpegRefused as csrc/ivit_jpeg_host.h refuses."""
    d = bytes(data)
    info, tabs, ri, pos = _parse(d)
    coefs = [np.zeros((n, 64), np.int16) for n in info.blocks]
    br = _Bits(d, pos)
    pred = [0] * info.ncomp
    mw, mh = info.mcus
    total, next_rst = mw * mh, 0
    q32 = info.qt.astype(np.int64)
    for mcu in range(total):
        if ri and mcu and mcu % ri == 0:
            m = br.next_marker()
            if m != 0xD0 + next_rst:
                raise _invalid("restart marker out of sequence")
            next_rst = (next_rst + 1) & 7
            pred = [0] * info.ncomp
        my, mx = divmod(mcu, mw)
        for c in range(info.ncomp):
            ch, cv = (info.hs, info.vs) if c == 0 else (1, 1)
            for by in range(cv):
                for bx in range(ch):
                    blk = coefs[c][(my * cv + by) * info.bw[c] + mx * ch + bx]
                    s = br.symbol(tabs[c][0])
                    diff = _extend(br.bits(s), s) if s else 0
                    pred[c] += diff
                    if not -32768 <= pred[c] <= 32767:
                        raise _invalid("DC coefficient outside 16 bits")
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.symbol(tabs[c][1])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 64:
                                raise _invalid("run past coefficient 63")
                            continue
                        k += r
                        if k > 63:
                            raise _invalid("run past coefficient 63")
                        blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                        k += 1
                    deq = blk.astype(np.int64) * q32[c]
                    col = np.abs(deq).reshape(8, 8).sum(0)
                    if col.max() > COLUMN_BOUND:
                        raise _unsupported("coefficients beyond 8-bit samples: a block column sums to %d (bound %d)" % (col.max(), COLUMN_BOUND))
                    if col.sum() > SUM_EXACT:
                        v = _idct_samples(deq[None])
                        if v.min() < -512 or v.max() > 511:
                            raise _unsupported("coefficients beyond 8-bit samples: a sample leaves the bound [-512, 511]")
    if br.next_marker() != 0xD9:
        raise _invalid("no EOI behind the last MCU")
    return info, coefs


# ---------------------------------------------------------------- the device half, as numpy
def _islow(x):
    """jidctint.c's 1-D pass on the last axis of an int64 array [..., 8], before the descale"""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i] for i in range(8))
    z1 = (x2 + x6) * 4433
    tmp2 = z1 + x6 * -15137
    tmp3 = z1 + x2 * 6270
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)


def _idct_samples(deq):
    """dequantised [blocks, 64] -> the samples before the range limit, int64 [blocks, 8, 8]"""
    x = deq.reshape(-1, 8, 8)
    ws = (_islow(x.transpose(0, 2, 1)) + (1 << 10)) >> 11                  # [block, column, row]
    return (_islow(ws.transpose(0, 2, 1)) + (1 << 17)) >> 18               # [block, row, column]


def idct_reference(coefs, qt):
    """int16 [blocks, 64], uint8 [64] -> uint8 [blocks, 8, 8]: dequantise, column pass descaled by 11 bits, row pass by 18, then
    libjpeg's range limit of the 10-bit masked value: the sign-extended 10 bits + 128, clamped to 0 .. 255"""
    v = _idct_samples(coefs.astype(np.int64) * qt.astype(np.int64)) & 1023
    v = np.where(v >= 512, v - 1024, v) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def _plane(blocks, bw, bh):
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample_reference(p, hs, vs, dw, dh, w, h):
    """a chroma plane (its first dh rows and dw columns are the subsampled image) -> int [h, w]"""
    p = p[:dh, :dw].astype(np.int64)
    if hs == 1:
        return p[:h, :w]
    if dw <= 2:                                                            # libjpeg keeps the fancy forms for planes wider than 2
        return np.repeat(np.repeat(p, vs, 0), 2, 1)[:h, :w]
    if vs == 2:
        up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        rows = np.empty((2 * dh, dw), np.int64)
        rows[0::2], rows[1::2] = 3 * p + up, 3 * p + dn
        left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
        out = np.empty((2 * dh, 2 * dw), np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
        return out[:h, :w]
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((dh, 2 * dw), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out[:h, :w]


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct_reference(info, coefs):
    """(JpegInfo, coefficients) -> uint8 [h, w, 3]"""
    planes = [_plane(idct_reference(coefs[c], info.qt[c]), info.bw[c], info.bh[c]) for c in range(info.ncomp)]
    w, h = info.w, info.h
    y = planes[0][:h, :w].astype(np.int64)
    if info.ncomp == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    dw, dh = -(-w // info.hs), -(-h // info.vs)
    cb = _upsample_reference(planes[1], info.hs, info.vs, dw, dh, w, h) - 128
    cr = _upsample_reference(planes[2], info.hs, info.vs, dw, dh, w, h) - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def jpeg_reference(data):
    """bytes of a JPEG file -> uint8 [h, w, 3], the bytes of PIL's Image.open(f).convert("RGB"); raises JpegRefused"""
    return reconstruct_reference(*jpeg_coefficients_reference(data))


# ---------------------------------------------------------------- the library's entries
def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


def _refusal(status, err):
    return JpegRefused(status, err.value.decode("ascii", "replace"))


def query(data):
    """one file -> (JpegDesc with its three offsets 0, coefficients (int16 elements), workspace bytes); no GPU call"""
    lib = _lib.load()
    desc, ncoef, nws, err = _lib.JpegDesc(), ctypes.c_int64(), ctypes.c_size_t(), ctypes.create_string_buffer(256)
    st = lib.ivit_jpeg_query_host(data, len(data), ctypes.byref(desc), ctypes.byref(ncoef), ctypes.byref(nws), err, len(err))
    if st != IVIT_OK:
        raise _refusal(st, err)
    return desc, ncoef.value, nws.value


def entropy_decode(data, out=None):
    """one file -> (JpegDesc, int16 numpy array of its coefficients, component after component); `out`: a caller's int16 array of at
    least that many elements (pinned memory, a slice of a staging buffer).  No GPU call; ctypes releases the GIL."""
    lib = _lib.load()
    desc, n, _ = query(data)
    if out is None:
        out = np.empty(n, np.int16)
    if out.dtype != np.int16 or out.ndim != 1 or out.size < n or not out.flags.c_contiguous:
        raise ValueError("out: a contiguous int16 array of at least %d elements" % n)
    err = ctypes.create_string_buffer(256)
    st = lib.ivit_jpeg_entropy_decode_host(data, len(data), ctypes.c_void_p(out.ctypes.data), n, err, len(err))
    if st != IVIT_OK:
        raise _refusal(st, err)
    return desc, out[:n]


def _align(n, a):
    return (n + a - 1) // a * a


def layout(descs, ncoefs, nws):
    """places B decoded files back to back: sets the three offsets of every descriptor (coefficients and planes at multiples of 16
    bytes) -> (table, coefficient elements, pixel bytes, workspace bytes)"""
    table = (_lib.JpegDesc * max(1, len(descs)))()
    co = po = wo = 0
    for i, d in enumerate(descs):
        ctypes.memmove(ctypes.byref(table[i]), ctypes.byref(d), ctypes.sizeof(_lib.JpegDesc))
        table[i].coef_offset, table[i].pixel_offset, table[i].plane_offset = co, po, wo
        co += _align(ncoefs[i], 8)
        po += d.w * d.h * 3
        wo += _align(nws[i], 16)
    return table, co, po, wo


def reconstruct(coefs, table, B, pixels, workspace, table_dev=None, h=None):
    """the device call: coefs int16 tensor, table the host JpegDesc array (layout), pixels / workspace uint8 tensors on the same
    device.  Asynchronous on the current stream; returns the device copy of the table (keep it alive until the work is done)."""
    import torch
    from .quant_modules import handle
    if table_dev is None:
        raw = np.frombuffer(table, np.uint8, B * ctypes.sizeof(_lib.JpegDesc)).copy() if B else np.zeros(0, np.uint8)
        table_dev = torch.from_numpy(raw).to(pixels.device)
    (h or handle(pixels.device)).call("ivit_jpeg_reconstruct_u8", ctypes.c_void_p(coefs.data_ptr()), ctypes.c_int64(coefs.numel()),
                                      ctypes.cast(table, ctypes.c_void_p), ctypes.c_void_p(table_dev.data_ptr()), int(B),
                                      ctypes.c_void_p(workspace.data_ptr()), ctypes.c_size_t(workspace.numel()),
                                      ctypes.c_void_p(pixels.data_ptr()), ctypes.c_size_t(pixels.numel()))
    return table_dev


def decode(files_or_bytes, device, threads=8, fallback="pil"):
    """paths or byte strings -> (RaggedImages on `device`, fallbacks): the entropy decode of every file on a pool of `threads` host
    threads (at most 16) into ONE pinned staging buffer, one copy, one reconstruction call.  A file the decoder refuses is decoded by
    PIL (`fallback="pil"`, PIL importable) and uploaded beside the others; `fallbacks` lists (index, reason) of those files.  With
    any other `fallback`, or without PIL, the first refusal raises JpegRefused with the library's reason."""
    import torch
    from .preprocess import DESC_DTYPE, RaggedImages
    datas = [_read(x) for x in files_or_bytes]
    if not datas:
        raise ValueError("no images")
    device = torch.device(device)
    threads = max(1, min(16, int(threads), len(datas)))
    info, fallbacks, pil_pixels = [None] * len(datas), [], {}

    def fall_back(i, e):
        if fallback != "pil":
            raise e
        try:
            from PIL import Image
        except ImportError:
            raise e
        import io
        pil_pixels[i] = np.array(Image.open(io.BytesIO(datas[i])).convert("RGB"))
        fallbacks.append((i, e.reason))

    for i, d in enumerate(datas):
        try:
            info[i] = query(d)
        except JpegRefused as e:
            fall_back(i, e)
    queried = [i for i in range(len(datas)) if info[i] is not None]
    table, ncoef, _, nws = layout([info[i][0] for i in queried], [info[i][1] for i in queried], [info[i][2] for i in queried])
    staging = torch.empty(max(1, ncoef), dtype=torch.int16)
    if device.type == "cuda":
        staging = staging.pin_memory()
    host = staging.numpy()

    def work(j):
        a = int(table[j].coef_offset)
        try:
            entropy_decode(datas[queried[j]], host[a:a + info[queried[j]][1]])
        except JpegRefused as e:                            # a refusal behind the headers: the stream itself
            return e
        return None

    if queried:
        with ThreadPoolExecutor(threads) as pool:
            refused = list(pool.map(work, range(len(queried))))
        for j, e in enumerate(refused):
            if e is not None:
                fall_back(queried[j], e)
    fallbacks.sort()
    # the pixel pool holds every image in the order given; the table keeps the files that decoded, where their coefficients lie
    desc = np.zeros(len(datas), DESC_DTYPE)
    off = 0
    for i in range(len(datas)):
        hh, ww = pil_pixels[i].shape[:2] if i in pil_pixels else (info[i][0].h, info[i][0].w)
        desc["h"][i], desc["w"][i], desc["offset"][i] = hh, ww, off
        off += hh * ww * 3
    native = [j for j in range(len(queried)) if queried[j] not in pil_pixels]
    final = (_lib.JpegDesc * max(1, len(native)))()
    wo = 0
    for k, j in enumerate(native):
        ctypes.memmove(ctypes.byref(final[k]), ctypes.byref(table[j]), ctypes.sizeof(_lib.JpegDesc))
        final[k].pixel_offset, final[k].plane_offset = int(desc["offset"][queried[j]]), wo
        wo += _align(info[queried[j]][2], 16)
    pixels = torch.empty(max(1, off), dtype=torch.uint8, device=device)
    for i, a in pil_pixels.items():
        o = int(desc["offset"][i])
        pixels[o:o + a.size] = torch.from_numpy(a.reshape(-1)).to(device)
    if native:
        coefs = staging.to(device, non_blocking=True)
        workspace = torch.empty(max(1, wo), dtype=torch.uint8, device=device)
        reconstruct(coefs, final, len(native), pixels, workspace)
        torch.cuda.current_stream(device).synchronize()         # the staging buffer, the table and the workspace die with this frame
    return RaggedImages(pixels[:off], desc), fallbacks
