#!/usr/bin/env python3
"""Time the pixel-format conversion on the KITTI shape (1241 x 376): 1536 device-resident frames (the batch of the
pyramid figure) of BGR8, BGRA8 and GRAY16 through svo_pyramid_set_upload_format_device into level 0 of a 1536-frame set,
without a lens and with the lens of tools/undistort_time.py (convert into the staging planes, then the remap).

Timing: hipEvents on the context stream (svo_ctx_event_record) around the one call; one untimed pass, then the median
of --reps passes.  Yardstick, in the same process: a plain device-to-device copy (torch, timed with its own events on
its own stream, same scheme) that moves as many bytes in total as the path reads plus writes, i.e. a copy of half that
many bytes.  That copy is the floor for any kernel with this traffic.  Traffic counted per pixel: the format's bytes in
and one byte out; with a lens the staging plane's byte written and read again and the output byte (the map's 6 bytes
per pixel are read once per thread and slice, not per image, and are not counted).

One frame of every result is compared with the numpy restatement (tests/convert_ref.py, tests/undistort_ref.py).
--per-thread runs the whole measurement once per value of SVO_CONVERT_PER_THREAD (images a thread walks), each in a
fresh process.  Prints one JSON line per run; --out also writes it to a file.

    python tools/convert_time.py [--frames 1536] [--reps 20] [--per-thread 1,2,4,8] [--out profiles/convert_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch  # (before libsvo_hip initialises HIP: torch's own HIP runtime then finds the GPU too)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1241, 376
LENS = (-2.32951777e-01, 6.17256346e-02, -1.83274571e-05, 3.39255772e-05, -7.54987702e-03)
FORMATS = (("bgr8", 3, torch.uint8), ("bgra8", 4, torch.uint8), ("gray16", 2, torch.int16))
PYRAMID_BUILD_MS = 0.80  # the pyramid build of 1536 frames of this shape, for scale


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def copy_ms(total_bytes, reps):
    """A device-to-device copy whose read plus write traffic is total_bytes."""
    n = total_bytes // 2
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for k in range(reps + 1):
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if k:
            ms.append(a.elapsed_time(b))
    del src, dst
    return median(ms)


def measure(frames, reps):
    import convert_ref as CR
    import svo_amd
    import undistort_ref as U
    ctx = svo_amd.default_context()
    k = svo_amd.PinholeCamera.kitti()
    plain = svo_amd.PinholeCamera(W, H, k.fx, k.fy, k.cx, k.cy)
    lens = svo_amd.PinholeCamera(W, H, k.fx, k.fy, k.cx, k.cy, *LENS)
    want_map = U.make_map(k.as_dict(), LENS)
    pset = svo_amd.PyramidSet(frames, W, H, 1)
    px = W * H * frames
    rows, copies = [], {}
    for fmt, bpp, dtype in FORMATS:
        shape = (frames, H, W) if fmt == "gray16" else (frames, H, W, bpp)
        lo, hi = (-32768, 32768) if fmt == "gray16" else (0, 256)
        raw = torch.randint(lo, hi, shape, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        for camera in (plain, lens):
            ms = []
            for rep in range(reps + 1):
                ctx.record(0)
                pset.upload_device(0, frames, raw.data_ptr(), camera, fmt, 8)
                ctx.record(1)
                if rep:
                    ms.append(ctx.elapsed_ms(0, 1))
            mid = frames // 2
            img = raw[mid].cpu().numpy()
            want = CR.convert_ref(img.view(np.uint16) if fmt == "gray16" else img, fmt, 8)
            if camera is lens:
                want = U.remap(want, *want_map)
            total = px * (bpp + 1 + (3 if camera is lens else 0))
            if total not in copies:
                copies[total] = copy_ms(total, reps)
            t = median(ms)
            rows.append({"format": fmt, "lens": camera is lens, "ms_median": t, "ms_min": min(ms), "ms_max": max(ms),
                         "bytes_total": total, "bytes_per_s": total / (t * 1e-3), "copy_ms_median": copies[total],
                         "copy_bytes_per_s": total / (copies[total] * 1e-3), "ratio_to_copy": t / copies[total],
                         "us_per_frame": t * 1e3 / frames, "ratio_to_pyramid_build": t / PYRAMID_BUILD_MS,
                         "gpu_equals_numpy": bool(np.array_equal(pset.download(mid, 0), want))})
        del raw
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                timeout=10).stdout.strip() or None
    except OSError:
        commit = None
    return {"tool": "convert_time", "width": W, "height": H, "frames": frames, "reps": reps,
            "per_thread": int(os.environ.get("SVO_CONVERT_PER_THREAD", "0")) or "default",
            "pyramid_build_ms": PYRAMID_BUILD_MS, "parent_commit": commit, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--per-thread", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.per_thread:
        for v in a.per_thread.split(","):
            env = dict(os.environ, SVO_CONVERT_PER_THREAD=str(int(v)))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--reps", str(a.reps)],
                               env=env, timeout=600)
            if r.returncode != 0:
                sys.exit(r.returncode)
        return
    line = json.dumps(measure(a.frames, a.reps))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
