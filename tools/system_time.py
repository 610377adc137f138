#!/usr/bin/env python3
"""Latency per frame of the tracker (svo_amd.System) on the KITTI shape: the band sequence of tests/system_scene.py at
1241 x 376 (same construction: four fronto-parallel bands, integer disparities per frame), 32 frames, KITTI intrinsics,
the reference's config (cell 30, patch 5, levels 0..3).  One untimed pass over the sequence first (code objects,
allocations), then --reps timed passes with a fresh System each.

Every step of a frame is a synchronous call (its results come back to the host), so the host clock around it includes
the device work and its synchronise.  Printed: milliseconds per frame, split by step (median and mean over the frames
that ran the step, over all timed passes): frame construction (upload + pyramid), align, reproject, candidates, depth
update, and on keyframes BA and selection; the whole add_image for tracked frames and for keyframes.  One JSON line.

The Python mirror (svo_amd.System) and the C++ mirror (svo_amd::System through build/svo_host_check system, one
process, its first pass untimed as well) are timed on the same frames with the same cell order and printed side by side:
every key once per mirror ("python", "cpp").

With --lens k1,k2,p1,p2,k3 the camera has that lens: the frames are made raw on the host first (tests/undistort_ref.py
distort_image) and the System undistorts them on the device, so "frame" then includes the remap.

With --pixel-format rgb8 (or bgr8, rgba8, bgra8) every frame is handed over as colour with R = G = B = the grey frame,
so the conversion on the device gives the same grey image and the same run, and "frame" then includes the conversion.

    python tools/system_time.py [--frames 32] [--reps 3] [--lens k1,k2,p1,p2,k3] [--pixel-format rgb8]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import system_scene as SC  # noqa: E402
import svo_amd  # noqa: E402
import svo_amd.synth as synth  # noqa: E402

HOST_CHECK = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "svo_host_check")

W, H = 1241, 376
STEPS = ("frame", "align", "reproject", "candidates", "depth", "ba", "select")


def one_pass(images, cfg):
    system = svo_amd.System(cfg, instrument=True)
    rows = []
    for k, img in enumerate(images):
        t0 = time.perf_counter()
        ok = system.add_image(img, k)
        total = time.perf_counter() - t0
        rows.append(dict(system.timings, total=total, result=system.last_result, status=system.status, ok=ok,
                         n_obs=system.cur_frame.number_observation()))
    return system, rows


def cpp_passes(images, cfg, cell_order, passes):
    """Rows like one_pass's from `passes` runs of the C++ mirror in one process, pass by pass."""
    with tempfile.TemporaryDirectory() as d:
        data, raw = synth.write_system_problem(cfg, images, cell_order, d)
        out = subprocess.run([HOST_CHECK, "system", data, raw, str(passes)], capture_output=True, text=True, check=True,
                             timeout=600).stdout.splitlines()
    rows, cur = [], []
    for k, line in enumerate(out):
        if line.startswith("frame "):
            f = [int(x) for x in line.split()[1:]]
            t = {a: float(b) for a, b in (x.split("=") for x in out[k + 3].split()[1:])}
            cur.append(dict(t, result=f[1], status=f[2], n_obs=f[4]))
        elif line == "trajectory":
            rows.append(cur)
            cur = []
    return rows


def summarise(rows, S):
    tracked = [r for r in rows if r["result"] == S.SUCCESS]
    keyfr = [r for r in rows if r["result"] == S.KEYFRAME]
    out = {"tracked_frames": len(tracked), "keyframes": len(keyfr), "failed": sum(r["result"] == S.FAILED for r in rows),
           "observations_median": statistics.median(r["n_obs"] for r in rows)}
    for name, group in (("tracked", tracked), ("keyframe", keyfr)):
        if group:
            out[f"{name}_total_ms_median"] = 1e3 * statistics.median(r["total"] for r in group)
            out[f"{name}_total_ms_mean"] = 1e3 * statistics.fmean(r["total"] for r in group)
    for step in STEPS:
        v = [r[step] for r in rows if step in r]
        if v:
            out[f"{step}_ms_median"] = 1e3 * statistics.median(v)
            out[f"{step}_ms_mean"] = 1e3 * statistics.fmean(v)
            out[f"{step}_calls"] = len(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lens", default="")
    ap.add_argument("--pixel-format", default="gray8", choices=("gray8", "bgr8", "rgb8", "bgra8", "rgba8"))
    a = ap.parse_args()
    images, _ = SC.make_sequence(a.frames, W, H)
    cfg = svo_amd.Config(desired_detected_points_for_initialization=1000)  # SSC keeps about half: ~500 of 546 cells
    lens = [float(v) for v in a.lens.split(",")] if a.lens else []
    if lens:
        import numpy as np
        import undistort_ref as U
        cam = dict(fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, width=W, height=H)
        images = np.stack([U.distort_image(img, cam, lens) for img in images])
        for k, v in enumerate(lens):
            setattr(cfg, "d%d" % k, v)
    if a.pixel_format != "gray8":
        import numpy as np
        from svo_amd._capi import PIXEL_SHAPES
        images = np.stack([images] * PIXEL_SHAPES[a.pixel_format][2], axis=-1)
        cfg.pixel_format = a.pixel_format
    one_pass(images, cfg)  # warm-up
    rows = []
    for _ in range(a.reps):
        system, r = one_pass(images, cfg)
        rows += r[2:]  # the frames processNewFrame handled
    S = svo_amd.System
    cpp = [r for p in cpp_passes(images, cfg, system.map.cell_orders, a.reps + 1)[1:] for r in p[2:]]
    out = {"tool": "system_time", "width": W, "height": H, "frames": a.frames, "reps": a.reps, "lens": lens,
           "pixel_format": a.pixel_format,
           "keyframes_in_map": system.map.size_keyframes(), "seeds": system.depth_estimator.number_filters(),
           "python": summarise(rows, S), "cpp": summarise(cpp, S)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
