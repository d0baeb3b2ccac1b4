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
