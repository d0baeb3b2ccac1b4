"""tests/golden/pil_views.npz (tools/make_pil_views_fixture.py) as the view tests read it: loaded once, left unchanged.  Its views
are over the images of tests/golden/pil_resize.npz (pil_fixture.fixture)."""
import functools

import numpy as np

from conftest import load_golden
from pil_fixture import fixture


@functools.lru_cache(maxsize=None)
def views_fixture():
    """-> (npz, images, groups): groups = [(crop, view table, PIL's bytes uint8 [n, crop, crop, 3])], one per crop, the views in the
    file's order"""
    from ivit_amd.views import make_views
    g = load_golden("pil_views.npz")
    images = fixture()[1]
    crops, sizes = g["crops"].astype(np.int64), g["crops"].astype(np.int64) ** 2 * 3
    offs = np.cumsum(sizes) - sizes
    groups = []
    for crop in sorted(set(crops.tolist()), reverse=True):
        sel = np.nonzero(crops == crop)[0]
        want = np.stack([g["bytes"][offs[j]:offs[j] + sizes[j]].reshape(crop, crop, 3) for j in sel])
        groups.append((int(crop), make_views(g["views"][sel]), want))
    return g, images, groups


def group_ids():
    return [f"crop{c}" for c, _, _ in views_fixture()[2]]


def entry_args(ims, views, crop, nchw, scale=0.03):
    """one call of ivit_view_transform_u8 (nchw) or ivit_view_resize_u8_pil over the images `ims`
    -> (entry, argument list in abi_cases' form, (image table, view table): the host copies the call validates)"""
    import ctypes
    from ivit_amd import _lib
    from ivit_amd import preprocess as pp
    from ivit_amd import views as vw
    sizes = np.array([im.size for im in ims], np.int64)
    desc = np.zeros(len(ims), pp.DESC_DTYPE)
    desc["offset"], desc["h"], desc["w"] = np.cumsum(sizes) - sizes, [im.shape[0] for im in ims], [im.shape[1] for im in ims]
    pixels = np.concatenate([im.reshape(-1) for im in ims])
    views = np.ascontiguousarray(views, dtype=vw.VIEW_DTYPE).copy()
    head = [("in", pixels), pixels.size, desc.ctypes.data_as(ctypes.POINTER(_lib.ImageDesc)), ("in", desc.view(np.uint8).copy()), len(ims),
            views.ctypes.data_as(ctypes.POINTER(_lib.ViewDesc)), ("in", views.view(np.uint8).copy()), len(views), crop]
    if nchw:
        mean, std = np.array(pp.IMAGENET_DEFAULT_MEAN, np.float32), np.array(pp.IMAGENET_DEFAULT_STD, np.float32)
        return "ivit_view_transform_u8", head + [("host", mean), ("host", std), scale, ("out", np.zeros((len(views), 3, crop, crop), np.int8))], (desc, views)
    return "ivit_view_resize_u8_pil", head + [("out", np.zeros((len(views), crop, crop, 3), np.uint8))], (desc, views)
