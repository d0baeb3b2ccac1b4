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


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("fname", ["micro_vit_b2.npz", "micro_swin_b2.npz"])
def test_side_outputs_follow_their_logits_buffer_through_an_eviction(fname):
    """predict / score / features (and a ViT's attention) keep their outputs beside the logits buffer of their (batch, slices): an
    uncaptured shape that left the workspace cache comes back with the same results on fresh buffers, a captured one never leaves."""
    cfg, eng = _engine(fname)
    vit = hasattr(eng, "attention")
    labels = lambda b: torch.arange(b, dtype=torch.int64, device="cuda") % cfg.num_classes
    buf, lab3 = dev(iv.make_images_int8(cfg, 3, seed=1)), labels(3)
    replays = {"predict": eng.capture_predict(buf, k=3, nstreams=2), "score": eng.capture_score(buf, lab3, nstreams=2),
               "features": eng.capture_features(buf, nstreams=2)}
    if vit:
        replays["attention"] = eng.capture_attention(buf, blocks=-1, nstreams=2)

    one, lab1 = dev(iv.make_images_int8(cfg, 1, seed=3)), labels(1)
    calls = {"predict": lambda x, lab, **kw: eng.predict(x, k=3, **kw), "score": lambda x, lab, **kw: eng.score(x, lab, **kw),
             "features": lambda x, lab, **kw: eng.features(x, **kw)}
    first = {name: f(one, lab1, copy=True) for name, f in calls.items()}
    for b in (2, 4, 5, 6, 7):                                              # with (1, 1): more shapes than the four that stay
        x = dev(iv.make_images_int8(cfg, b, seed=40 + b))
        for f in calls.values():
            f(x, labels(b))
    assert (1, 1) not in eng._native_ws
    for name, f in calls.items():
        again = f(one, lab1)
        if name != "features":                                             # features without logits leaves last_logits alone
            assert eng.last_logits is eng._native_buffers(1, 1)[1], name
        torch.cuda.synchronize()
        assert _same(again, first[name]), name
    assert eng.last_logits is eng._native_buffers(1, 1)[1]

    imgs = dev(iv.make_images_int8(cfg, 3, seed=2))
    buf.copy_(imgs)
    calls["attention"] = lambda x, lab, **kw: eng.attention(x, blocks=-1, **kw)
    for name, replay in replays.items():
        got = tuple(t.clone() for t in replay())                           # the eager call below writes the same buffers
        torch.cuda.synchronize()
        assert _same(got, calls[name](imgs, lab3, nslices=2, copy=True)), name
    assert (3, 2) in eng._graph_keys and len(eng._native_ws.unpinned()) <= 4
