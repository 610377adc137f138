#!/usr/bin/env python3
"""Time svo_klt_track on the KITTI shape: 64 frame pairs x 2000 points at 1241 x 376, window 11, 4 levels, 30
iterations (what algorithm::computeOpticalFlowSparse asks of cv::calcOpticalFlowPyrLK), with hipEvents on the context
stream around the whole synchronous call (uploads of the point arrays, the kernel, downloads), and the numpy
restatement of the contract (tests/klt_ref.py) on one of those pairs on the CPU.  Prints one JSON line.

    python tools/klt_time.py [--pairs 64] [--points 2000] [--reps 10]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import klt_ref as K  # noqa: E402
import svo_amd  # noqa: E402

W, H, WIN, LEVELS, VIEWS = 1241, 376, 11, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    tex = K.Texture(77)
    shifts = [(2.3 * k, -1.1 * k) for k in range(VIEWS + 1)]
    views = [tex.render(W, H, s) for s in shifts]
    ref_set = svo_amd.PyramidSet(VIEWS, W, H, LEVELS)
    cur_set = svo_amd.PyramidSet(VIEWS, W, H, LEVELS)
    ref_set.upload(0, np.stack(views[:VIEWS]))
    cur_set.upload(0, np.stack(views[1:]))
    ref_set.build()
    cur_set.build()
    frames = np.array([[p % VIEWS, p % VIEWS] for p in range(a.pairs)], np.int32)
    off = np.arange(a.pairs + 1, dtype=np.int32) * a.points
    px = np.stack([rng.uniform(8.0, W - 9.0, a.pairs * a.points), rng.uniform(8.0, H - 9.0, a.pairs * a.points)], axis=1)
    ctx = svo_amd.default_context()

    def call():
        return svo_amd.klt_track_batch(ref_set, cur_set, frames, off, px, px, WIN, LEVELS - 1, 30, 1e-4, 1e-4, trace=True)
    for _ in range(2):
        cur, status, _, trace = call()
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.record(0)
        call()
        ctx.record(1)
        ms.append(ctx.elapsed_ms(0, 1))
        wall.append((time.perf_counter() - t0) * 1e3)
    n = a.points
    rp = [ref_set.download(0, l) for l in range(LEVELS)]
    cp = [cur_set.download(0, l) for l in range(LEVELS)]
    t0 = time.perf_counter()
    want = K.klt_track(rp, cp, px[:n], px[:n], WIN, LEVELS - 1, 30, 1e-4, 1e-4)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    match = bool(cur[:n].tobytes() == want[0].tobytes() and np.array_equal(status[:n], want[1]) and
                 np.array_equal(trace[:n], want[2]))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                timeout=10).stdout.strip() or None
    except OSError:
        commit = None
    ms.sort()
    wall.sort()
    print(json.dumps({"tool": "klt_time", "pairs": a.pairs, "points_per_pair": a.points, "width": W, "height": H,
                      "win": WIN, "levels": LEVELS, "reps": a.reps, "event_ms_median": ms[len(ms) // 2],
                      "event_ms_min": ms[0], "event_ms_max": ms[-1], "wall_ms_median": wall[len(wall) // 2],
                      "points_per_s": a.pairs * a.points / (ms[len(ms) // 2] * 1e-3),
                      "tracked_fraction": float(status.mean()), "mean_iterations_level0": float(trace[:, 0, 0].mean()),
                      "numpy_one_pair_ms": cpu_ms, "numpy_points": n, "gpu_equals_numpy_on_that_pair": match,
                      "parent_commit": commit}))


if __name__ == "__main__":
    main()
