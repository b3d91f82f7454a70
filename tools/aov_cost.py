#!/usr/bin/env python3
"""What the rt_aov_film planes cost on a full-size frame, and how far the fast mode's film is from the parity mode's in
units of the per-pixel standard error.

    python tools/aov_cost.py [--workload c4] [--reps 2] [--out DIR]

Renders the workload through rt_render_aov_device (film and planes in torch tensors) with: no planes, only rgb_sq_sum,
every plane with aov_spp = 16, every plane with aov_spp = 0 (all samples); one warm-up frame, then --reps timed frames
of each, alternating.  Then (--sigma) C3 in both precisions with the second moment: |f32 - f64| / SE_f64 per pixel and
channel.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sigma", action="store_true", help="also the f32-vs-f64 distance in standard errors (C3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    import rustraytracer_amd as rr
    from rustraytracer_amd import _ffi as F

    ctx = rr.Context(0)
    dev = torch.device("cuda", 0)

    def setup(name):
        preset, kw, W, H, spp, _ = bench.WORKLOADS[name]
        sc = rr.Scene(preset, W / H, **kw)
        return sc, ctx.upload(sc), W, H, spp

    def buffers(W, H, names):
        planes = {}
        for k in names:
            shape = rr.api._plane_shape(k, H, W)
            planes[k] = torch.zeros(shape, device=dev, dtype=torch.float64 if rr.AOV_PLANES[k][2] is np.float64 else torch.int32)
        return (torch.zeros((H, W, 3), dtype=torch.float64, device=dev), torch.zeros((H, W), dtype=torch.int32, device=dev),
                planes)

    sc, gs, W, H, spp = setup(a.workload)
    variants = [("none", (), 0), ("rgb_sq", ("rgb_sq",), 0), ("all_aov16", tuple(rr.AOV_PLANES), 16),
                ("all_aov0", tuple(rr.AOV_PLANES), 0)]
    bufs = {v[0]: buffers(W, H, v[1]) for v in variants}
    cfg = rr.make_cfg(W, H, spp, seed=1)
    res = {v[0]: [] for v in variants}
    for rep in range(a.reps + 1):
        for name, names, aov_spp in variants:
            d_rgb, d_n, planes = bufs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st, ms = ctx.render_aov_device(gs, sc.camera, cfg, d_rgb, d_n, planes, aov_spp=aov_spp)
            wall = (time.perf_counter() - t0) * 1e3
            if rep > 0:  # rep 0 warms every variant up
                res[name].append({"wall_ms": wall, "kernel_ms": st.kernel_ms, "aov_ms": ms, "rays": st.rays})
    base = bufs["none"]
    for name, names, aov_spp in variants:
        d_rgb, d_n, planes = bufs[name]
        same = bool(torch.equal(d_rgb, base[0]) and torch.equal(d_n, base[1]))
        r = res[name]
        print(json.dumps({"workload": a.workload, "variant": name, "aov_spp": aov_spp, "film_equals_no_planes": same,
                          "wall_ms": [round(x["wall_ms"], 1) for x in r], "kernel_ms": [round(x["kernel_ms"], 1) for x in r],
                          "aov_ms": [round(x["aov_ms"], 2) for x in r], "rays": r[0]["rays"]}), flush=True)
    gs.close()
    sc.close()
    if a.sigma:
        sc, gs, W, H, spp = setup("c3")
        out = {}
        for prec, label in ((F.RT_PRECISION_F64, "f64"), (F.RT_PRECISION_F32, "f32")):
            d_rgb, d_n, planes = buffers(W, H, ("rgb_sq",))
            ctx.render_aov_device(gs, sc.camera, rr.make_cfg(W, H, spp, seed=1, precision=prec), d_rgb, d_n, planes)
            out[label] = (d_rgb.cpu().numpy(), d_n.cpu().numpy().astype(np.uint32), planes["rgb_sq"].cpu().numpy())
        s64, n64, q64 = out["f64"]
        s32 = out["f32"][0]
        se = rr.standard_error(s64, q64, n64) * n64[..., None]  # standard error of the SUM (film units)
        z = np.abs(s32 - s64) / np.where(se > 0, se, np.nan)
        zf = z[np.isfinite(z)]
        q = np.percentile(zf, [50, 90, 99, 99.9]).tolist() if zf.size else []
        print(json.dumps({"workload": "c3", "spp": spp, "what": "|f32 - f64| / SE_f64 per pixel and channel",
                          "finite": int(zf.size), "zero_variance": int((~np.isfinite(z)).sum()),
                          "p50_p90_p99_p999": [round(x, 3) for x in q], "max": round(float(zf.max()), 3) if zf.size else None,
                          "frac_above_3": round(float((zf > 3).mean()), 5) if zf.size else None,
                          "gaussian_p50_p90_p99_p999": [0.674, 1.645, 2.576, 3.291]}), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            np.save(os.path.join(a.out, "c3_z.npy"), z.astype(np.float32))
        gs.close()
    ctx.close()


if __name__ == "__main__":
    main()
