"""tests/golden/pil_resize.npz (tools/make_pil_resize_fixture.py) as the PIL-resize tests read it: loaded once, left unchanged."""
import functools

import numpy as np

from conftest import load_golden


@functools.lru_cache(maxsize=None)
def fixture():
    g = load_golden("pil_resize.npz")
    shapes, offsets, pixels = g["shapes"], g["offsets"], g["pixels"]
    images = [pixels[o:o + int(h) * int(w) * 3].reshape(int(h), int(w), 3) for o, (h, w) in zip(offsets, shapes)]
    cases = [(int(s), int(c), [int(i) for i in g[f"case{k}_images"]], g[f"case{k}_out"]) for k, (s, c) in enumerate(g["cases"])]
    return g, images, cases


def case_ids():
    return [f"size{s}-crop{c}" for s, c, _, _ in fixture()[2]]


def entry_args(ims, size, crop, nchw, scale=0.03):
    """one call of ivit_eval_transform_u8 (nchw) or ivit_resize_center_crop_u8_pil on the ragged batch `ims`
    -> (entry, argument list in abi_cases' form, keep-alive: the host descriptor table the call validates)"""
    import ctypes
    from ivit_amd import _lib
    from ivit_amd import preprocess as pp
    sizes = np.array([im.size for im in ims], np.int64)
    desc = np.zeros(len(ims), pp.DESC_DTYPE)
    desc["offset"], desc["h"], desc["w"] = np.cumsum(sizes) - sizes, [im.shape[0] for im in ims], [im.shape[1] for im in ims]
    pixels = np.concatenate([im.reshape(-1) for im in ims])
    head = [("in", pixels), pixels.size, desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)), ("in", desc.view(np.uint8).copy()),
            len(ims), size, crop]
    if nchw:
        mean, std = np.array(pp.IMAGENET_DEFAULT_MEAN, np.float32), np.array(pp.IMAGENET_DEFAULT_STD, np.float32)
        return "ivit_eval_transform_u8", head + [("host", mean), ("host", std), scale, ("out", np.zeros((len(ims), 3, crop, crop), np.int8))], desc
    return "ivit_resize_center_crop_u8_pil", head + [("out", np.zeros((len(ims), crop, crop, 3), np.uint8))], desc
