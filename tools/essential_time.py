#!/usr/bin/env python3
"""Time svo_essential_ransac on 64 frame pairs x 2000 matches with 30 % outliers (threshold 1 px, confidence 0.999, at
most 1000 samples: what algorithm::computeEssentialMatrix asks of cv::findEssentialMat), with hipEvents on the context
stream around the whole synchronous call (uploads, the sampling rounds with their host walks, downloads), and the
numpy restatement of the contract (tests/essential_ref.py) on one of those pairs on the CPU.  Prints one JSON line.

    python tools/essential_time.py [--pairs 64] [--matches 2000] [--reps 10]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_ref as R  # noqa: E402
import two_view_ref as T  # noqa: E402
import svo_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    scenes = [R.with_outliers(T.make_scene(100 + p, a.matches, "side", noise=0.3), 0.3, 500 + p) for p in range(a.pairs)]
    off = np.arange(a.pairs + 1, dtype=np.int32) * a.matches
    ref_px = np.concatenate([s.ref_px for s in scenes])
    cur_px = np.concatenate([s.cur_px for s in scenes])
    cam = svo_amd.PinholeCamera.kitti()
    ctx = svo_amd.default_context()

    def call():
        return svo_amd.essential_ransac_batch(cam, off, ref_px, cur_px, 1.0, 0.999, 1000, a.seed)
    for _ in range(2):
        r = call()
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.record(0)
        call()
        ctx.record(1)
        ms.append(ctx.elapsed_ms(0, 1))
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = R.ransac(scenes[0].ref_px, scenes[0].cur_px, 1.0, 0.999, 1000, a.seed, pair=0)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    n = a.matches
    match = bool(r.iterations[0] == want.iterations and r.n_inliers[0] == want.n_inliers and
                 np.array_equal(r.mask[:n], want.mask) and int(r.best[0][0]) == want.best[0])
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                timeout=10).stdout.strip() or None
    except OSError:
        commit = None
    ms.sort()
    wall.sort()
    print(json.dumps({"tool": "essential_time", "pairs": a.pairs, "matches_per_pair": a.matches, "outlier_share": 0.3,
                      "reps": a.reps, "event_ms_median": ms[len(ms) // 2], "event_ms_min": ms[0], "event_ms_max": ms[-1],
                      "wall_ms_median": wall[len(wall) // 2], "pairs_per_s": a.pairs / (ms[len(ms) // 2] * 1e-3),
                      "mean_samples": float(r.iterations.mean()), "max_samples": int(r.iterations.max()),
                      "mean_inlier_share": float(r.n_inliers.mean() / a.matches), "failed_pairs": int((r.status != 0).sum()),
                      "numpy_one_pair_ms": cpu_ms, "gpu_equals_numpy_on_that_pair": match, "parent_commit": commit}))


if __name__ == "__main__":
    main()
