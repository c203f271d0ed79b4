#!/usr/bin/env python3
"""Device-event timing of tdt_raycast_device (the ray-query kernel, csrc/tdt_query.hip) on two loads:

  camera  the 1920x1080 primary rays (sample 0) of the bench frame: bench.py's default workload, scene config 2 (64^3) and
          host.camera_reference_pose(1920, 1080, 64, 8)
  random  2M random rays (origins in and around the box, normalised directions) through the 512^3 BASELINE scene (config 5)

    python tools/raycast_time.py [--reps 20] [--warmup 3] [--json out.json]

Rays and hits live in torch tensors on cuda:0; each repetition is one tdt_raycast_device call bracketed by HIP events on the
context's stream.  Prints one JSON line per load: median / min ms and rays per second (median).  Measurement only: no test
and no bench.py number depends on it."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_load(name, scene, rays, reps, warmup):
    import torch
    from tdt4230_project_raytracing_amd import rt
    stream = torch.cuda.Stream(device=0)
    ctx = rt.Context(0, stream=stream.cuda_stream)
    try:
        vbos = rt.upload_scene(ctx, scene)
        dev = rays.to("cuda:0").contiguous()
        out = torch.empty((dev.shape[0], 64), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        L = rt.lib()
        call = lambda: ctx.check(L.tdt_raycast_device(ctx.h, ctypes.c_void_p(dev.data_ptr()), dev.shape[0], ctypes.c_void_p(out.data_ptr())))  # noqa: E731
        for _ in range(warmup):
            call()
        ctx.finish()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        hits = rt.hits_from_bytes(out)
        med = float(np.median(ms))
        res = {"load": name, "rays": int(dev.shape[0]), "median_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4),
               "rays_per_s": round(dev.shape[0] / (med * 1e-3), 0), "reps": reps,
               "hit_fraction": round(float((hits["status"] == rt.RAY_HIT).mean()), 4),
               "iter_limit_fraction": round(float((hits["status"] == rt.RAY_ITER_LIMIT).mean()), 4),
               "mean_iterations": round(float(hits["iterations"].mean()), 2)}
        del vbos
        return res
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from tdt4230_project_raytracing_amd import host, rt

    # the bench frame's camera rays: the library's own pick of every pixel, sample 0
    scene = host.Scene.config(2)
    cam = host.camera_reference_pose(1920, 1080, 64, 8)
    r = rt.Renderer(scene, cam)
    try:
        xy = np.stack(np.meshgrid(np.arange(1920), np.arange(1080)), -1).reshape(-1, 2).astype(np.int32)
        _, cam_rays = r.pick(xy, 0, return_rays=True)
    finally:
        r.close()
    results = [time_load("camera_1080p_config2", scene, torch.from_numpy(cam_rays), args.reps, args.warmup)]

    big = host.Scene.config(5)
    rng = np.random.default_rng(12345)
    n = 2 * 1024 * 1024
    of = big.blobs[6]
    mn, scale = of[:3].astype(np.float64), float(of[4])
    o = rng.uniform(-0.2, 1.2, (n, 3)) * scale + mn
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32))
    results.append(time_load("random_2M_config5_512", big, rays, args.reps, args.warmup))
    for res in results:
        print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
