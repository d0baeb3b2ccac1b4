"""Run under torch.distributed.run with N ranks (gloo or nccl): every rank receives the broadcast integer constants
(ivit_amd.dist.build_engine_broadcast) and runs ivit_amd.predict.evaluate on ITS shard (ivit_amd.dist.shard_range) of one seeded
batch, in batches of 3; the hit counts meet in the one all_reduce that ends evaluate.  Labels are the class each image's own
prediction ranks 1st, 3rd, 6th, by turns, so the expected counts are known.  Rank 0 also evaluates the whole batch alone and
prints `EVAL_CHECK_OK world W n N correct {...}` when the reduced counts equal both; every rank exits non-zero otherwise.  With
one GPU all ranks share device 0 (IVIT_DIST_BACKEND=gloo): the sharding and the reduction are what is tested, not the scaling.
Used by tests/test_predict_gpu.py::test_evaluate_sharded_over_two_ranks."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivit_amd as iv  # noqa: E402
from ivit_amd import dist as ivdist  # noqa: E402
from ivit_amd.predict import evaluate  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = os.environ.get("IVIT_DIST_BACKEND", "nccl")
    local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    dist.init_process_group(backend, rank=rank, world_size=world)
    name, total = sys.argv[1], int(sys.argv[2])
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", name))
    cfg = iv.CONFIGS[str(g["cfg_name"])]
    scales = {k[len("scale/"):]: np.float32(g[k]) for k in g.files if k.startswith("scale/")}
    weights = iv.make_vit_weights(cfg, int(g["seed"])) if rank == 0 else None       # only rank 0 owns the weights
    eng = ivdist.build_engine_broadcast(cfg, weights, scales, device, rank, world)
    images = torch.from_numpy(iv.make_images_int8(cfg, total, seed=77)).to(device)
    topk = (1, 5)
    k = min(6, cfg.num_classes)
    order = eng.predict(images, k=k, copy=True)[0].cpu().numpy()
    ranks = np.array([(0, 2, k - 1)[i % 3] for i in range(total)])
    labels = torch.from_numpy(order[np.arange(total), ranks].astype(np.int64))
    expect = {j: int((ranks < j).sum()) for j in topk}
    out = ivdist.evaluate_sharded(eng, images, labels, 3, rank, world, topk=topk)
    ok = out["n"] == total and out["correct"] == expect
    if rank == 0:
        alone = evaluate(eng, [(images[a:a + 3], labels[a:a + 3]) for a in range(0, total, 3)], topk=topk)
        ok = ok and alone == out
        print(f"EVAL_CHECK_{'OK' if ok else 'FAIL'} world {world} n {out['n']} correct {out['correct']} expected {expect} "
              f"shards {[ivdist.shard_range(total, r, world) for r in range(world)]} backend {backend}", flush=True)
    on = device if backend == "nccl" else "cpu"
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=on)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) else 1)


if __name__ == "__main__":
    main()
