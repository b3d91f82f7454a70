#!/usr/bin/env python3
"""Several ranks (one process each) on ONE GPU render the auxiliary planes of rt_aov_film for their interleaved tiles
(rt_render_aov with tile_rank / tile_world), FilmGather.gather_planes (rustraytracer_amd/dist.py) collects them on rank 0
over gloo, and rank 0 compares them with its own one-rank render bit for bit.

Launch:  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
             --master-port 29531 tools/aov_mp_check.py
Prints one JSON line on rank 0; exit code 0 = identical.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import torch.distributed as dist

    import rustraytracer_amd as rr
    from rustraytracer_amd import dist as rd

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo")
    W, H, spp = 48, 32, 8
    sc = rr.cornell_box_statue(W / H, mesh_faces=3000, variant=1)
    ctx = rr.Context(0)
    gs = ctx.upload(sc)
    r = ctx.render_aov(gs, sc.camera, rr.make_cfg(W, H, spp, seed=4, tile_rank=rank, tile_world=world), aov_spp=4)
    names = list(r.planes)
    planes = [torch.from_numpy(r.planes[k].astype(np.int64) if r.planes[k].dtype == np.uint32 else r.planes[k])
              for k in names]
    rd.FilmGather(W, H, "cpu").gather_planes(*planes)
    ok = True
    if rank == 0:
        full = ctx.render_aov(gs, sc.camera, rr.make_cfg(W, H, spp, seed=4), aov_spp=4)
        ok = all(np.array_equal(p.numpy().astype(full.planes[k].dtype), full.planes[k]) for k, p in zip(names, planes))
        print(json.dumps({"ranks": world, "planes": names, "bit_identical": bool(ok), "image": [W, H, spp]}), flush=True)
    gs.close()
    ctx.close()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
