"""numpy restatement of the pixel-format contract (include/svo_c.h, "pixel formats"), with explicit shifts.

colour   Y = (4899 R + 9617 G + 1868 B + 8192) >> 14      (alpha ignored)
gray16   Y = min(255, v >> shift)
gray8    a copy
"""
import numpy as np

BPP = {"gray8": 1, "bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4, "gray16": 2}
FORMATS = tuple(BPP)


def luma(r, g, b):
    r, g, b = (np.asarray(v).astype(np.uint32) for v in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def convert_ref(img, pixel_format, shift=8):
    """(.., h, w[, channels]) in the format's dtype -> (.., h, w) uint8."""
    a = np.asarray(img)
    if pixel_format == "gray8":
        assert a.dtype == np.uint8
        return a.copy()
    if pixel_format == "gray16":
        assert a.dtype == np.uint16 and 0 <= shift <= 8
        return np.minimum(a.astype(np.uint32) >> shift, 255).astype(np.uint8)
    assert a.dtype == np.uint8 and a.shape[-1] == BPP[pixel_format]
    if pixel_format in ("bgr8", "bgra8"):
        return luma(a[..., 2], a[..., 1], a[..., 0])
    return luma(a[..., 0], a[..., 1], a[..., 2])


def layout_bytes(pixel_format, width, height, count, row_stride=0, image_stride=0):
    """The bytes a call reads: image_stride*(count-1) + row_stride*(height-1) + width*bpp, strides resolved."""
    row = width * BPP[pixel_format]
    rs = row_stride or row
    ims = image_stride or rs * height
    return ims * (count - 1) + rs * (height - 1) + row if count else 0


def from_bytes(buf, pixel_format, width, height, count, row_stride=0, image_stride=0):
    """The (count, h, w[, channels]) images a padded byte buffer holds in that layout (a copy)."""
    bpp = BPP[pixel_format]
    rs = row_stride or width * bpp
    ims = image_stride or rs * height
    buf = np.asarray(buf, np.uint8)
    rows = np.stack([np.stack([buf[k * ims + y * rs: k * ims + y * rs + width * bpp] for y in range(height)])
                     for k in range(count)])
    if pixel_format == "gray16":
        return rows.view(np.uint16).reshape(count, height, width)
    return rows.reshape(count, height, width) if bpp == 1 else rows.reshape(count, height, width, bpp)
