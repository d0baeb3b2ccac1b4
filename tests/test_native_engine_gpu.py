"""The workspace cache of both engines under a captured graph: more shapes than the cache keeps pass through it, and the graph's
own shape stays where the graph left it."""
import numpy as np
import pytest

from conftest import load_golden, golden_scales

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ivit_amd as iv  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine(fname):
    g = load_golden(fname)
    if str(g["cfg_name"]) in iv.SWIN_CONFIGS:
        from ivit_amd.swin_engine import SwinEngine
        cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
        return cfg, SwinEngine(cfg, iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g))
    from ivit_amd.engine import ViTEngine
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    return cfg, ViTEngine.from_float(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_captured_shape_survives_more_shapes_than_the_cache_keeps(fname):
    cfg, eng = _engine(fname)
    buf = dev(iv.make_images_int8(cfg, 3, seed=1))
    replay = eng.capture(buf, nstreams=2)
    for b in (1, 2, 4, 5, 6, 7):                                           # six other shapes: more than the four that stay
        eng.forward(dev(iv.make_images_int8(cfg, b, seed=40 + b)))
    imgs = dev(iv.make_images_int8(cfg, 3, seed=2))
    buf.copy_(imgs)
    got = replay()
    torch.cuda.synchronize()
    assert torch.equal(got, eng.forward(imgs, copy=True))
    assert eng._native_buffers(3, 2)[1] is got
    assert len(eng._native_ws.unpinned()) <= 4 and (3, 2) in eng._graph_keys
