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
