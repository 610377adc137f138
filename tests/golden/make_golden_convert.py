"""A colour fixture for the pixel-format conversion: a textured RGB crop of the reference's own test image
tests/test_data/images/image_1.png (1920 x 1080, 8-bit RGB), with its offset.  Runs only where the reference tree is;
the tests read the committed convert_rgb_crop.npz alone.

  rgb      (192, 256, 3) uint8: the decoded bytes of the window, untouched
  offset   (row, column) of the window in the image

The window is the one with the largest sum of absolute horizontal differences of the green channel among the windows
on a 64-pixel grid (a street texture, not sky).  tests/test_convert.py holds the crop's grey image against the same
window of refimages.npz["image_1"], which make_golden_refimages.py built from the whole image.

usage: python3 tests/golden/make_golden_convert.py [reference root]
"""
import os
import sys

import numpy as np
from PIL import Image

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "convert_rgb_crop.npz")
H, W, GRID = 192, 256, 64

if __name__ == "__main__":
    rgb = np.asarray(Image.open(os.path.join(REF, "tests/test_data/images/image_1.png")).convert("RGB"), dtype=np.uint8)
    texture = np.abs(np.diff(rgb[..., 1].astype(np.int32), axis=1))
    best = max(((int(texture[r:r + H, c:c + W - 1].sum()), r, c)
                for r in range(0, rgb.shape[0] - H + 1, GRID) for c in range(0, rgb.shape[1] - W + 1, GRID)),
               key=lambda t: (t[0], -t[1], -t[2]))
    _, r, c = best
    np.savez_compressed(OUT, rgb=np.ascontiguousarray(rgb[r:r + H, c:c + W]), offset=np.array([r, c], np.int32))
    print("window at", (r, c), "texture", best[0], "wrote", OUT, os.path.getsize(OUT), "bytes")
