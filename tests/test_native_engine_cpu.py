"""The engines' shared base without a device: the workspace cache's policy, the constants both freezers emit (guarded by
digests, the way synth's weights are), and that the four ways into a runner are written once, on NativeEngine."""
import hashlib
import inspect

from conftest import load_golden, golden_scales
import ivit_amd as iv
from ivit_amd.engine import ViTEngine, pack_constants
from ivit_amd.native import NativeEngine, ShapeCache, SideOutputs
from ivit_amd.swin_engine import SwinEngine, freeze_swin, pack_swin_constants


def test_shape_cache_policy():
    made = []

    def make(*key):
        made.append(key)
        return object()
    c = ShapeCache(make)
    first = c.get((1, 1))
    assert c.get((1, 1)) is first and made == [(1, 1)]                     # same key: same object, no second build
    for b in (2, 3, 4):
        c.get((b, 1))
    assert c.unpinned() == [(1, 1), (2, 1), (3, 1), (4, 1)] and len(made) == 4
    c.get((5, 1))                                                          # the fifth unpinned key: the oldest one leaves
    assert (1, 1) not in c and c.unpinned() == [(2, 1), (3, 1), (4, 1), (5, 1)]
    assert c.get((1, 1)) is not first and made[-1] == (1, 1) and len(made) == 6        # ... and is built again on request
    assert (2, 1) not in c
    # a pinned key survives any number of later keys, and does not count toward the four
    pinned = c.get((3, 1))
    c.pin((3, 1))
    c.get((9, 2))
    c.pin((9, 2))
    for b in range(10, 30):
        c.get((b, 1))
        assert len(c.unpinned()) <= 4
    assert c.get((3, 1)) is pinned and (9, 2) in c
    assert c.unpinned() == [(26, 1), (27, 1), (28, 1), (29, 1)]
    assert sum(k == (3, 1) for k in made) == 1 and sum(k == (9, 2) for k in made) == 1


def test_side_outputs_policy():
    made = []

    def make():
        made.append(object())
        return made[-1]
    ws = ShapeCache(lambda *key: object())                                 # the logits buffers, plain objects
    s = SideOutputs(ws)
    first = s.get((1, 1, 5), ws.get((1, 1)), make)
    assert s.get((1, 1, 5), ws.get((1, 1)), make) is first and len(made) == 1          # same key, same logits: no second build
    assert s.get((1, 1, 3), ws.get((1, 1)), make) is not first and len(made) == 2       # another key beside the same logits
    captured = s.get((9, 2, 5), ws.get((9, 2)), make)
    s.pin((9, 2, 5))                                                       # a graph pins the side outputs and their workspace entry
    ws.pin((9, 2))
    for b in (2, 3, 4):
        s.get((b, 1, 5), ws.get((b, 1)), make)
    assert (1, 1) in ws and set(s.items) == {(1, 1, 5), (1, 1, 3), (9, 2, 5), (2, 1, 5), (3, 1, 5), (4, 1, 5)}
    n = len(made)
    assert s.get((2, 1, 5), ws.get((2, 1)), make) is made[n - 3] and len(made) == n    # a hit drops nothing and builds nothing
    # the fifth unpinned shape evicts (1, 1): the next build drops exactly its two entries — not (9, 2), pinned, nor the cached shapes
    s.get((5, 1, 5), ws.get((5, 1)), make)
    assert (1, 1) not in ws and set(s.items) == {(9, 2, 5), (2, 1, 5), (3, 1, 5), (4, 1, 5), (5, 1, 5)}
    # (1, 1) comes back on a new logits object (and evicts (2, 1)): built again, never the tensors of the old buffer
    again = s.get((1, 1, 5), ws.get((1, 1)), make)
    assert again is not first and again is made[-1] and (2, 1, 5) not in s.items and (3, 1, 5) in s.items
    # the same key beside another logits object: a rebuild, although the key is present
    n = len(made)
    assert s.get((1, 1, 5), object(), make) is made[-1] and len(made) == n + 1
    # a pinned entry survives any number of later keys, also one whose shape the workspace cache no longer holds
    gone = s.get((30, 1), ws.get((30, 1)), make)
    s.pin((30, 1))
    for b in range(10, 30):
        s.get((b, 1), ws.get((b, 1)), make)
        assert len([k for k in s.items if k not in s.pinned]) <= 5         # the four cached shapes and the one being built
    assert (30, 1) not in ws and s.items[(30, 1)][1] is gone
    assert s.get((9, 2, 5), ws.get((9, 2)), make) is captured


def _digest(blob, table, host):
    h = hashlib.sha256(blob.tobytes())
    h.update(repr(sorted(table.items())).encode())
    h.update(repr(sorted(host.items())).encode())
    return h.hexdigest()


# recorded from the freezers as they stood before they shared `linear` / `norm` and freeze_swin moved to freeze.py
FROZEN_SHA256 = {
    "vit": "3a6acddedc746d1b070c09f20ee73145fcba249d489375d38af3524b669beda8",
    "swin": "5319fce01e323f98cb26bf35bb669224bdf13018c281d3ebcce182b3b3b2e4fa",
    "swin_exp_tables": "9f9c18cb33161bf036aa22947774531e8d083d1e38c3a9113265823b361d2b79",
}


def frozen_digests():
    g = load_golden("micro_vit_b2.npz")
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    consts, f32 = iv.freeze.freeze_vit(cfg, iv.make_vit_weights(cfg, int(g["seed"])), golden_scales(g))
    out = {"vit": _digest(*pack_constants(consts), {k: float(v) for k, v in f32.items()})}
    g = load_golden("micro_swin_b2.npz")
    cfg = iv.SWIN_CONFIGS[str(g["cfg_name"])]
    w, sc = iv.make_swin_weights(cfg, int(g["seed"])), golden_scales(g)
    out["swin"] = _digest(*pack_swin_constants(freeze_swin(cfg, w, sc)))
    out["swin_exp_tables"] = _digest(*pack_swin_constants(freeze_swin(cfg, w, sc, exp_tables=True)))
    return out


def test_freezers_emit_the_recorded_constants():
    assert iv.freeze.freeze_swin is freeze_swin
    assert frozen_digests() == FROZEN_SHA256


def test_entry_points_are_defined_once():
    assert issubclass(ViTEngine, NativeEngine) and issubclass(SwinEngine, NativeEngine)
    for name in ("forward", "capture", "predict", "capture_predict", "score", "capture_score", "features", "capture_features",
                 "head_scale_host"):
        assert name in NativeEngine.__dict__ and name not in ViTEngine.__dict__ and name not in SwinEngine.__dict__, name
        assert getattr(ViTEngine, name) is getattr(SwinEngine, name) is NativeEngine.__dict__[name], name
        assert inspect.signature(getattr(ViTEngine, name)) == inspect.signature(getattr(SwinEngine, name)), name
