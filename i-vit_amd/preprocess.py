"""Device side of the reference's eval transform (utils/data_utils.py:82-92) after the PIL resize + centre
crop: ToTensor -> Normalize(IMAGENET_DEFAULT_MEAN/STD) -> the model's input QuantAct, in one kernel from
uint8 HWC pixels.  The host ships 150 KB per 224x224 image instead of 602 KB of fp32."""
import ctypes

import numpy as np
import torch

from . import _lib
from .quant_modules import handle

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def normalize_quantize(u8_hwc, scale, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
    """u8_hwc: uint8 device tensor [B, H, W, 3]; scale: the input QuantAct's scale (qact_input).
    Returns int8 [B, 3, H, W] — what `model(...)` / `engine.forward(...)` take."""
    if u8_hwc.dtype != torch.uint8 or u8_hwc.dim() != 4 or u8_hwc.shape[-1] != 3:
        raise TypeError("expected a uint8 tensor [B, H, W, 3]")
    x = u8_hwc.contiguous()
    B, H, W, _ = x.shape
    out = torch.empty(B, 3, H, W, dtype=torch.int8, device=x.device)
    m = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in mean])
    s = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in std])
    handle(x.device).call("ivit_normalize_quantize_u8", ctypes.c_void_p(x.data_ptr()), B, H, W, m, s,
                          float(np.float32(scale)), ctypes.c_void_p(out.data_ptr()))
    return out


def resize_center_crop(u8_hwc, size=256, crop=224):
    """Resize(size, bicubic) + CenterCrop(crop) on the device (utils/data_utils.py:82-88; the reference uses
    size = int(crop / 0.875)): uint8 [B, H0, W0, 3] -> uint8 [B, crop, crop, 3]."""
    if u8_hwc.dtype != torch.uint8 or u8_hwc.dim() != 4 or u8_hwc.shape[-1] != 3:
        raise TypeError("expected a uint8 tensor [B, H, W, 3]")
    x = u8_hwc.contiguous()
    B, H0, W0, _ = x.shape
    ws = torch.empty(B * H0 * crop * 3, dtype=torch.float32, device=x.device)
    out = torch.empty(B, crop, crop, 3, dtype=torch.uint8, device=x.device)
    handle(x.device).call("ivit_resize_center_crop_u8", ctypes.c_void_p(x.data_ptr()), B, H0, W0, int(size), int(crop),
                          ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    return out


def eval_transform(u8_hwc, scale, size=256, crop=224):
    """the whole eval transform of the reference on the device: resize -> centre crop -> ToTensor -> Normalize -> input QuantAct"""
    return normalize_quantize(resize_center_crop(u8_hwc, size, crop), scale)


# ---------------------------------------------------------------- the PIL-pinned front end on ragged batches
# The reference's eval transform works on PIL images (utils/data_utils.py:82-92: transforms.Resize(size, interpolation=3),
# transforms.CenterCrop), and PIL's bicubic is not torch's: uint8 images are resampled in 22-bit fixed point with a uint8
# intermediate between the horizontal and the vertical pass.  `pil_resize_center_crop_reference` states that arithmetic once, in
# numpy; csrc/ivit_preprocess.h restates it on the device; tests/golden/pil_resize.npz (written by PIL) pins both.
DESC_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])        # struct ivit_image_desc


def resized_size(h, w, size):
    """torchvision Resize(int): the shorter side becomes `size`, the longer int(size * long / short), in integers -> (Hr, Wr)"""
    h, w, size = int(h), int(w), int(size)
    return (size, size * w // h) if h <= w else (size * h // w, size)


def crop_offset(dim, crop):
    """torchvision CenterCrop: rint((dim - crop) / 2.0), ties to even"""
    return int(np.rint((int(dim) - int(crop)) / 2.0))


def _pil_bicubic(x):
    a = -0.5
    x = np.abs(x)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        outer = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def pil_coefficients(in_size, out_size, i):
    """PIL's taps of output index i along one axis (input length in_size, output length out_size): (xmin, k int64 [n]),
    k the 22-bit fixed-point coefficients.  All in float64, in PIL's operation order."""
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, np.float64(1.0))
    support = np.float64(2.0) * fs
    ss = np.float64(1.0) / fs
    center = (np.float64(i) + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)                       # int(): truncation, as the C conversion
    n = min(int(center + support + 0.5), int(in_size)) - xmin
    if n <= 0:
        return xmin, np.zeros(0, np.int64)
    w = _pil_bicubic((np.arange(n, dtype=np.int64) + xmin - center + 0.5) * ss)
    ww = np.cumsum(w)[-1]                                            # sequential, ascending j, from 0.0 (0.0 + w_0 == w_0)
    if ww != 0.0:
        w = w / ww
    k = np.where(w < 0.0, np.trunc(-0.5 + w * 4194304.0), np.trunc(0.5 + w * 4194304.0)).astype(np.int64)
    return xmin, k


def _pil_pass(src, in_size, out_size, first, count):
    """one pass along axis 0 of src (uint8 [in_size, ...]) for the output indices first .. first + count -> uint8 [count, ...]"""
    if in_size == out_size:
        return src[first:first + count].copy()
    out = np.empty((count,) + src.shape[1:], np.uint8)
    for o in range(count):
        xmin, k = pil_coefficients(in_size, out_size, first + o)
        acc = np.tensordot(k, src[xmin:xmin + len(k)].astype(np.int64), axes=(0, 0)) + (1 << 21)
        out[o] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def pil_resize_center_crop_reference(images, size, crop):
    """The contract of ivit_resize_center_crop_u8_pil in numpy: a list of uint8 [h, w, 3] arrays -> uint8 [B, crop, crop, 3],
    the bytes of PIL's Image.resize((Wr, Hr), Image.BICUBIC) then the centre crop.  Horizontal pass first, into uint8, for the
    cropped columns and the input rows the cropped rows' vertical taps reach; then the vertical pass; an axis whose length does
    not change is copied."""
    out = np.empty((len(images), crop, crop, 3), np.uint8)
    for b, im in enumerate(images):
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
        h, w = im.shape[:2]
        Hr, Wr = resized_size(h, w, size)
        if crop > Hr or crop > Wr:
            raise ValueError(f"image {b}: crop {crop} larger than the resized image {Hr} x {Wr}")
        top, left = crop_offset(Hr, crop), crop_offset(Wr, crop)
        if Hr == h:
            y0, y1 = top, top + crop
        else:
            lo, hi = pil_coefficients(h, Hr, top), pil_coefficients(h, Hr, top + crop - 1)
            y0, y1 = lo[0], hi[0] + len(hi[1])
        rows = np.ascontiguousarray(im[y0:y1].transpose(1, 0, 2))                     # [w, rows, 3]
        hor = _pil_pass(rows, w, Wr, left, crop).transpose(1, 0, 2)                     # [rows, crop, 3]
        if Hr == h:
            out[b] = hor
        else:
            full = np.zeros((h, crop, 3), np.uint8)
            full[y0:y1] = hor
            out[b] = _pil_pass(full, h, Hr, top, crop)
    return out


class RaggedImages:
    """a batch of uint8 HWC images of different sizes on the device: `pixels` the flat uint8 tensor, `desc` the descriptor table
    (numpy, DESC_DTYPE: what the calls validate), `desc_dev` its device copy (what the kernel reads)"""
    def __init__(self, pixels, desc, desc_dev=None):
        self.pixels, self.desc = pixels, np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        self.desc_dev = desc_dev if desc_dev is not None else torch.from_numpy(self.desc.view(np.uint8).copy()).to(pixels.device)

    def __len__(self):
        return len(self.desc)

    def __getitem__(self, sl):
        """a contiguous slice of the batch over the same pixel buffer and the same device table: no copy, no upload"""
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("RaggedImages takes contiguous slices")
        a, b, _ = sl.indices(len(self.desc))
        b = max(a, b)
        return RaggedImages(self.pixels, self.desc[a:b], self.desc_dev[a * DESC_DTYPE.itemsize:b * DESC_DTYPE.itemsize])


def pack_images(images, device):
    """list of uint8 [h, w, 3] arrays or tensors -> RaggedImages on `device`: the images back to back in one buffer, one upload"""
    arrs = []
    for im in images:
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise TypeError("expected uint8 images [h, w, 3]")
        arrs.append(np.ascontiguousarray(a))
    if not arrs:
        raise ValueError("no images")
    desc = np.zeros(len(arrs), DESC_DTYPE)
    desc["h"], desc["w"] = [a.shape[0] for a in arrs], [a.shape[1] for a in arrs]
    sizes = np.array([a.size for a in arrs], np.int64)
    desc["offset"] = np.cumsum(sizes) - sizes
    flat = np.concatenate([a.reshape(-1) for a in arrs])
    return RaggedImages(torch.from_numpy(flat).to(device), desc)


def _ragged_args(batch):
    if not isinstance(batch, RaggedImages) or len(batch) == 0:
        raise TypeError("expected a non-empty RaggedImages (pack_images)")
    return (ctypes.c_void_p(batch.pixels.data_ptr()), ctypes.c_size_t(batch.pixels.numel()),
            batch.desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)), ctypes.c_void_p(batch.desc_dev.data_ptr()), len(batch))


def resize_center_crop_pil(batch, size=256, crop=224):
    """Resize(size, bicubic) + CenterCrop(crop) as PIL computes them (utils/data_utils.py:82-88), one launch for the whole ragged
    batch: RaggedImages -> uint8 [B, crop, crop, 3]"""
    out = torch.empty(len(batch), crop, crop, 3, dtype=torch.uint8, device=batch.pixels.device)
    handle(out.device).call("ivit_resize_center_crop_u8_pil", *_ragged_args(batch), int(size), int(crop), ctypes.c_void_p(out.data_ptr()))
    return out


def eval_transform_pil(batch, scale, size=256, crop=224, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
    """the whole eval transform of the reference (utils/data_utils.py:82-92, then the input QuantAct) on a ragged batch in one
    launch, on PIL's bytes: RaggedImages -> int8 [B, 3, crop, crop]"""
    out = torch.empty(len(batch), 3, crop, crop, dtype=torch.int8, device=batch.pixels.device)
    m = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in mean])
    s = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in std])
    handle(out.device).call("ivit_eval_transform_u8", *_ragged_args(batch), int(size), int(crop), m, s,
                            float(np.float32(scale)), ctypes.c_void_p(out.data_ptr()))
    return out
