"""Writes tests/golden/jpeg.npz with Pillow: JPEG byte strings and the bytes of Image.open(f).convert("RGB"), the pin of
ivit_amd/jpeg.py and include/ivit_jpeg.h.  Small images chosen for the edges: sizes around the 8- and 16-pixel block and MCU sides and
around the two-sample width below which libjpeg replicates chroma, noise and a gradient, qualities 30 / 85 / 100, the three
subsamplings and grey, optimised tables, restart intervals, a long APP segment and bytes behind EOI, streams without JFIF, and the
refusals (progressive, CMYK, crafted headers, truncations, coefficients beyond 8-bit samples).

    python tools/make_jpeg_golden.py            # needs Pillow; rewrites the file

Keys: `accepted`, `refused` (names), `refused_status` (IVIT_ERR_* per refused name), `refused_reason` (a word of the message),
`jpg_<name>` uint8, `rgb_<name>` uint8 [h, w, 3] (accepted, and refused files that PIL decodes)."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 9), (8, 8), (9, 7), (16, 16), (17, 33), (53, 37), (64, 48)]         # (w, h)
SMALL = [(2, 2), (3, 5), (4, 3), (5, 2), (6, 6), (33, 1), (1, 19)]                       # around the two-sample chroma width
INVALID, UNSUPPORTED = 1, 3              # IVIT_ERR_INVALID, IVIT_ERR_UNSUPPORTED (include/ivit.h)


def picture(kind, w, h, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(1, w - 1), (y * 255) // max(1, h - 1), ((x + y) * 255) // max(1, w + h - 2)], -1).astype(np.uint8)


def encode(arr, mode="RGB", **kw):
    im = Image.fromarray(arr).convert(mode) if mode != "RGB" else Image.fromarray(arr)
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def segments(data):
    """[(marker, start of FF, end)] of the header segments up to and including SOS"""
    out, pos = [], 2
    while True:
        m, L = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.append((m, pos, pos + 2 + L))
        pos += 2 + L
        if m == 0xDA:
            return out


def patch_dqt(data, value):
    d = bytearray(data)
    for m, a, b in segments(data):
        if m == 0xDB:
            i = a + 4
            while i < b:
                d[i + 1:i + 65] = bytes([value]) * 64
                i += 65
    return bytes(d)


def dqt16(data):
    out, pos = bytearray(data[:2]), 2
    for m, a, b in segments(data):
        if m == 0xDB:
            body, i = bytearray(), a + 4
            while i < b:
                body += bytes([0x10 | data[i]]) + b"".join(bytes([0, v]) for v in data[i + 1:i + 65])
                i += 65
            out += bytes([0xFF, 0xDB, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
        else:
            out += data[a:b]
        pos = b
    return bytes(out + data[pos:])


def without_jfif(data, insert=b""):
    segs = segments(data)
    assert segs[0][0] == 0xE0
    return data[:2] + insert + data[segs[0][2]:]


def adobe(transform):
    body = b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform])
    return bytes([0xFF, 0xEE, 0, len(body) + 2]) + body


def patch_sof(data, offset, value, marker=None):
    d = bytearray(data)
    for m, a, b in segments(data):
        if m in (0xC0, 0xC1):
            if marker is not None:
                d[a + 1] = marker
            if offset is not None:
                d[a + 4 + offset] = value
    return bytes(d)


def main():
    acc, ref = {}, {}
    seed = 0
    for (w, h) in SIZES:
        for kind, quality in (("noise", 30), ("noise", 85), ("noise", 100), ("grad", 30), ("grad", 85), ("grad", 100)):
            arr = picture(kind, w, h, seed)
            seed += 1
            for sub in (0, 1, 2):
                acc["%dx%d_%s_q%d_s%d" % (w, h, kind, quality, sub)] = encode(arr, quality=quality, subsampling=sub)
            acc["%dx%d_%s_q%d_grey" % (w, h, kind, quality)] = encode(arr, "L", quality=quality)
    for (w, h) in SMALL:
        arr = picture("noise", w, h, seed)
        seed += 1
        for sub in (0, 1, 2):
            acc["%dx%d_noise_q85_s%d" % (w, h, sub)] = encode(arr, quality=85, subsampling=sub)
    arr = picture("noise", 53, 37, 1000)
    for sub in (0, 1, 2):
        acc["opt_s%d" % sub] = encode(arr, quality=85, subsampling=sub, optimize=True)
        for r in (1, 2):
            acc["rst%d_s%d" % (r, sub)] = encode(arr, quality=85, subsampling=sub, restart_marker_blocks=r)
    acc["opt_grey"] = encode(arr, "L", quality=85, optimize=True)
    acc["rst1_grey"] = encode(arr, "L", quality=85, restart_marker_blocks=1)
    acc["rst_rows_s2"] = encode(arr, quality=85, subsampling=2, restart_marker_rows=1)
    base = encode(picture("noise", 17, 33, 1001), quality=85, subsampling=2)
    app = bytes([0xFF, 0xE5, 0xFF, 0xFF]) + bytes(65533) + bytes([0xFF, 0xFE, 0, 5]) + b"hi!" + b"\xff\xff"   # APP5, COM, fill bytes
    acc["long_app_trailing"] = base[:2] + app + base[2:] + b"bytes behind EOI \xff\xd8\xff"
    acc["no_jfif"] = without_jfif(encode(picture("noise", 16, 16, 1002), quality=85, subsampling=0))
    acc["adobe_ycc"] = without_jfif(encode(picture("noise", 16, 16, 1003), quality=85, subsampling=0), adobe(1))
    acc["sof1"] = patch_sof(encode(picture("noise", 16, 16, 1004), quality=85, subsampling=2), None, 0, marker=0xC1)
    acc["q100_noise_big"] = encode(picture("noise", 64, 48, 1005), quality=100, subsampling=0)
    acc["extremes_q100"] = encode((np.indices((48, 64)).sum(0) % 2 * 255).astype(np.uint8)[:, :, None].repeat(3, 2), quality=100, subsampling=0)

    small = encode(picture("noise", 8, 8, 1006), quality=85, subsampling=0)
    src = picture("noise", 16, 16, 1007)
    ref["progressive"] = (encode(src, quality=85, progressive=True), UNSUPPORTED, "progressive")
    ref["cmyk"] = (encode(src, "CMYK", quality=85), UNSUPPORTED, "4 components")
    ref["sampling_4x1"] = (patch_sof(encode(src, quality=85, subsampling=0), 7, 0x41), UNSUPPORTED, "sampling")
    ref["adobe_rgb"] = (without_jfif(encode(src, quality=85, subsampling=0), adobe(0)), UNSUPPORTED, "RGB")
    ref["arithmetic"] = (patch_sof(encode(src, quality=85), None, 0, marker=0xC9), UNSUPPORTED, "arithmetic")
    ref["lossless"] = (patch_sof(encode(src, quality=85), None, 0, marker=0xC3), UNSUPPORTED, "lossless")
    ref["twelve_bit"] = (patch_sof(encode(src, quality=85), 0, 12), UNSUPPORTED, "12-bit")
    ref["dqt16"] = (dqt16(encode(src, quality=85)), UNSUPPORTED, "16-bit")
    ref["dqt255"] = (patch_dqt(encode(picture("noise", 17, 33, 1008), quality=30, subsampling=2), 255), UNSUPPORTED, "bound")
    for n in (0, 1, 2, 3, 20, len(small) // 2, len(small) - 40, len(small) - 3, len(small) - 2, len(small) - 1):
        ref["trunc_%d" % n] = (small[:n], INVALID, "")
    ref["no_soi"] = (b"\x00" + small[1:], INVALID, "SOI")
    segs = segments(small)
    dht = [s for s in segs if s[0] == 0xC4][0]
    ref["missing_dht"] = (small[:dht[1]] + small[segs[-1][1]:], INVALID, "Huffman table")
    dq = [s for s in segs if s[0] == 0xDB][0]
    ref["missing_dqt"] = (small[:dq[1]] + small[dq[2]:], INVALID, "quantisation table")
    bad = bytearray(small)
    bad[dq[1] + 3] += 1
    ref["bad_length"] = (bytes(bad), INVALID, "")
    r1 = bytearray(acc["rst1_s0"])
    i = r1.index(b"\xff\xd1")
    r1[i + 1] = 0xD3
    ref["restart_out_of_sequence"] = (bytes(r1), INVALID, "restart")

    out = {"accepted": np.array(sorted(acc)), "refused": np.array(sorted(ref)),
           "refused_status": np.array([ref[k][1] for k in sorted(ref)], np.int32), "refused_reason": np.array([ref[k][2] for k in sorted(ref)])}
    for k, v in acc.items():
        out["jpg_" + k] = np.frombuffer(v, np.uint8)
        out["rgb_" + k] = pil_rgb(v)
    for k, (v, _, _) in ref.items():
        out["jpg_" + k] = np.frombuffer(v, np.uint8)
    out["rgb_dqt255"] = pil_rgb(ref["dqt255"][0])
    path = os.path.join(ROOT, "tests", "golden", "jpeg.npz")
    np.savez_compressed(path, **out)
    print("%s: %d accepted, %d refused, %d bytes" % (path, len(acc), len(ref), os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
