#!/usr/bin/env python3
"""Time the undistortion step on the KITTI shape (1241 x 376) with hipEvents on the context stream:
  map creation, once (svo_undistort_map_create, after a warm-up on another camera has loaded the code object);
  one raw image from device memory into level 0 of a one-frame set (svo_pyramid_set_upload_undistort_device);
  1536 raw images (the benchmark's frame count) from device memory into a 1536-frame set through one map;
  the achieved bytes/s of both against the image bytes read plus written (2 x count x width x height; the map's
  6 bytes per pixel are reported beside it, they are read once per thread and slice, not once per image);
  the numpy restatement (tests/undistort_ref.py) on one image, and whether the device equals it.
The lens is the reference's test camera's (tests/test_camera.cpp:111).  --sweep runs the whole measurement once per
value of SVO_UNDISTORT_PER_THREAD (images a remap thread walks with its map entries), each in a fresh process.
Prints one JSON line per measurement.

    python tools/undistort_time.py [--frames 1536] [--reps 10] [--sweep 1,2,4,8,16]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch  # (before libsvo_hip initialises HIP: torch's own HIP runtime then finds the GPU too)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1241, 376
LENS = (-2.32951777e-01, 6.17256346e-02, -1.83274571e-05, 3.39255772e-05, -7.54987702e-03)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(frames, reps):
    import svo_amd
    import undistort_ref as U
    ctx = svo_amd.default_context()
    k = svo_amd.PinholeCamera.kitti()
    svo_amd.UndistortMap(svo_amd.PinholeCamera(64, 48, 32.0, 32.0, 31.5, 23.5, 0.1)).download()  # warm-up
    camera = svo_amd.PinholeCamera(W, H, k.fx, k.fy, k.cx, k.cy, *LENS)
    ctx.synchronize()
    ctx.record(0)
    m = camera.undistort_map(ctx)
    ctx.record(1)
    map_ms = ctx.elapsed_ms(0, 1)

    raw = torch.randint(0, 256, (frames, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    one = svo_amd.PyramidSet(1, W, H, 1)
    many = svo_amd.PyramidSet(frames, W, H, 1)

    def timed(pset, count):
        for _ in range(2):
            pset.upload_device(0, count, raw.data_ptr(), camera)
        ctx.synchronize()
        ms = []
        for _ in range(reps):
            ctx.record(0)
            pset.upload_device(0, count, raw.data_ptr(), camera)
            ctx.record(1)
            ms.append(ctx.elapsed_ms(0, 1))
        return ms

    one_ms, many_ms = timed(one, 1), timed(many, frames)
    img = raw[frames // 2].cpu().numpy()
    cam = dict(k.as_dict())
    t0 = time.perf_counter()
    want_map = U.make_map(cam, LENS)
    numpy_map_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want = U.remap(img, *want_map)
    numpy_remap_ms = (time.perf_counter() - t0) * 1e3
    xy, frac = m.download()
    match = bool(np.array_equal(many.download(frames // 2, 0), want) and np.array_equal(xy[..., 0], want_map[0]) and
                 np.array_equal(xy[..., 1], want_map[1]) and np.array_equal(frac, U.pack_frac(*want_map[2:])))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                timeout=10).stdout.strip() or None
    except OSError:
        commit = None
    px = W * H
    print(json.dumps({"tool": "undistort_time", "width": W, "height": H, "frames": frames, "reps": reps,
                      "per_thread": int(os.environ.get("SVO_UNDISTORT_PER_THREAD", "0")) or "default",
                      "map_create_ms": map_ms, "one_image_ms_median": median(one_ms), "one_image_ms_min": min(one_ms),
                      "one_image_image_bytes_per_s": 2 * px / (median(one_ms) * 1e-3),
                      "batch_ms_median": median(many_ms), "batch_ms_min": min(many_ms), "batch_ms_max": max(many_ms),
                      "batch_us_per_image": median(many_ms) * 1e3 / frames,
                      "batch_image_bytes_per_s": 2 * px * frames / (median(many_ms) * 1e-3),
                      "map_bytes": 6 * px, "numpy_map_ms": numpy_map_ms, "numpy_remap_one_image_ms": numpy_remap_ms,
                      "gpu_equals_numpy": match, "parent_commit": commit}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()
    if not a.sweep:
        return measure(a.frames, a.reps)
    for v in a.sweep.split(","):
        env = dict(os.environ, SVO_UNDISTORT_PER_THREAD=str(int(v)))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--reps", str(a.reps)],
                           env=env, timeout=600)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
