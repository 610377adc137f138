"""The undistortion anchor: the one recorded OpenCV result the reference ships (run where the reference tree exists;
the tests read only the committed .npz).

  tests/test_data/camera/undistort_input.png   1280 x 960 RGB, the input of tests/test_camera.cpp:115
  tests/test_data/camera/undistort_ref.png     the recorded PinholeCamera::undistortImage output (:120)

The fixture holds the GREEN channel of both (a channel, not a grey conversion: cv::remap works per channel, so the
recorded channel is what the contract must reproduce) and the camera and coefficients of tests/test_camera.cpp:107-111.

usage: python3 tests/golden/make_golden_undistort.py <reference root>
"""
import os
import sys

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "undistort_ref.npz")
CAMERA = np.array([560.33468243, 561.37973145, 651.26269237, 499.06652492, 1280, 960], np.float64)  # fx fy cx cy w h
DIST = np.array([-2.32951777e-01, 6.17256346e-02, -1.83274571e-05, 3.39255772e-05, -7.54987702e-03], np.float64)


def green(path):
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)[..., 1])


if __name__ == "__main__":
    ref = sys.argv[1]
    data = {"input_g": green(os.path.join(ref, "tests/test_data/camera/undistort_input.png")),
            "ref_g": green(os.path.join(ref, "tests/test_data/camera/undistort_ref.png")),
            "camera": CAMERA, "dist": DIST}
    np.savez_compressed(OUT, **data)
    for k, v in data.items():
        print(k, v.shape, v.dtype)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
