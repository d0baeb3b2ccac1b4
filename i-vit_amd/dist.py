"""Multi-GPU: one process per GPU, images sharded by rank, NO per-step collective.
The only collective is one broadcast of the packed integer constants (int8 weights,
int32 biases, dyadic tables, int16 position embedding) from rank 0 — RCCL over xGMI
on GPUs (`nccl` backend), gloo on CPU for the tests.
"""
import numpy as np
import torch
import torch.distributed as dist

from .engine import ViTEngine, frozen_vit, pack_constants
from .freeze import freeze_swin, freeze_vit  # noqa: F401  (names this module has always had)
from .swin_engine import SwinEngine, pack_swin_constants, packed_swin  # noqa: F401


def broadcast_packed(packed, rank, world, device):
    """(blob, table, host) of any engine from rank 0 to every rank: the table / host scalars as one small
    object, the byte blob as ONE tensor broadcast (RCCL ring over xGMI on GPUs)."""
    if world == 1:
        blob, table, host = packed
        return torch.from_numpy(blob).to(device), table, host
    meta, blob_t = [None], None
    if rank == 0:
        blob, table, host = packed
        meta = [(table, host, int(blob.size))]
        blob_t = torch.from_numpy(blob).to(device)
    dist.broadcast_object_list(meta, src=0)
    table, host, nbytes = meta[0]
    if rank != 0:
        blob_t = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dist.broadcast(blob_t, src=0)
    return blob_t, table, host


def broadcast_constants(consts, f32, rank, world, device):
    """rank 0 passes (consts, f32); other ranks pass (None, None).
    Returns (blob tensor on `device`, table, f32) on every rank."""
    packed = pack_constants(consts) + ({k: float(np.float32(v)) for k, v in f32.items()},) if rank == 0 else None
    return broadcast_packed(packed, rank, world, device)


def shard_range(total, rank, world):
    """contiguous, balanced split of `total` images over `world` ranks."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def build_engine_broadcast(cfg, weights, scales, device, rank, world):
    consts = f32 = None
    if rank == 0:
        consts, f32 = frozen_vit(cfg, weights, scales)
    blob, table, f32 = broadcast_constants(consts, f32, rank, world, device)
    return ViTEngine(cfg, None, f32, device=device, blob=blob, table=table)


def build_swin_engine_broadcast(cfg, weights, scales, device, rank, world):
    packed = packed_swin(cfg, weights, scales) if rank == 0 else None
    return SwinEngine(cfg, None, None, device=device, packed=broadcast_packed(packed, rank, world, device))


def evaluate_sharded(engine, images, labels, batch, rank, world, topk=(1, 5), transform=None, loss=False):
    """ivit_amd.predict.evaluate over THIS rank's contiguous share (shard_range) of `images` / `labels`, in batches of `batch`:
    every rank predicts its own images, its labels are uploaded once, and the hit counts meet in the one all_reduce that ends
    evaluate — no collective and no host-device copy per step.  loss=True adds the reference's `Loss` (evaluate's loss=True).
    Returns the reduced result on every rank."""
    from .predict import evaluate
    lo, hi = shard_range(len(labels), rank, world)
    if getattr(engine, "device", None) is not None:      # this rank's labels go up once: no copy inside evaluate's loop
        labels = torch.as_tensor(labels)[lo:hi].to(engine.device)
        lo, hi, images = 0, hi - lo, images[lo:hi]
    batches = ((images[a:min(a + batch, hi)], labels[a:min(a + batch, hi)]) for a in range(lo, hi, batch))
    return evaluate(engine, batches, topk=topk, transform=transform, rank=rank, world=world, loss=loss)


def probe_fit_sharded(engine, images, labels, batch, rank, world, num_classes, ridge=1e-3, transform=None, stats=None):
    """ivit_amd.predict.probe_fit over THIS rank's contiguous share (shard_range) of `images` / `labels`, in batches of `batch`:
    every rank accumulates the statistics of its own images (its labels uploaded once, no collective and no host-device copy per
    step), ONE all_reduce (sum) of the three int64 tensors joins them — exact integers: the same bits on every rank as one process
    over all the images — and every rank solves the same small system.  Returns the Head on every rank.  `stats`: the caller's own
    ZEROED ProbeStats to add into; it holds the reduced statistics afterwards (`probe.fit` refits from them with another ridge)."""
    from .probe import ProbeStats, fit
    lo, hi = shard_range(len(labels), rank, world)
    mine = torch.as_tensor(labels)[lo:hi].to(device=engine.device, dtype=torch.int64)
    if stats is None:
        stats = ProbeStats(engine.num_features, num_classes, engine.device)
    for a in range(lo, hi, batch):
        b = min(a + batch, hi)
        x = images[a:b]
        engine.probe_accumulate(transform(x) if transform is not None else x, mine[a - lo:b - lo], stats)
    if world > 1:
        stats.all_reduce()
    return fit(stats, engine.feature_scale_host(), ridge)


def kmeans_fit_sharded(engine, images, batch, rank, world, cent0, iters=20, transform=None):
    """exact integer k-means (ivit_amd.cluster.KMeans) over THIS rank's contiguous share (shard_range) of `images`, from the
    centroids `cent0` int8 [K, num_features] every rank passes alike (seed them once — `cluster.init_centroids` with one generator —
    or broadcast rank 0's): the rank embeds its images once (`predict.embed8`, the int8 features kept), and every iteration is assign
    and accumulate over its own rows, ONE all_reduce (sum) of sum, count and inertia — exact integers: the same bits on every rank
    as one process over all the images — and the same update everywhere.  Returns (kmeans, feat8 of this rank, inertia_history)."""
    from .cluster import KMeans
    from .predict import embed8
    lo, hi = shard_range(len(images), rank, world)
    feat8, _ = embed8(engine, (images[a:min(a + batch, hi)] for a in range(lo, hi, batch)), transform)
    km = KMeans(cent0.shape[0], engine.num_features, engine.device).set_centroids(cent0)
    km.world = world
    return km, feat8, km.fit(feat8, iters=iters)
