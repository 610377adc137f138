"""numpy restatement of the undistortion contract of include/svo_c.h (svo_undistort_*): the fixed-point map, the
integer bilinear remap with a zero border, and the two host point helpers.

Every map operation is one rounded IEEE double operation in the order the contract writes it (numpy's elementwise
arithmetic does not contract), so the map equals the device's in every entry.
"""
import numpy as np

ITERATIONS = 40  # undistorted_pixel's fixed-point iterations (part of the contract: SVO_UNDISTORT_POINT_ITERATIONS)


def raw_uv(cam, d, width=None, height=None):
    """The unrounded (u, v) of the contract for every output pixel: two (h, w) float64 arrays."""
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    w = cam["width"] if width is None else width
    h = cam["height"] if height is None else height
    k1, k2, p1, p2, k3 = (np.float64(v) for v in d)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    x = np.broadcast_to((j - cx) / fx, (h, w))
    y = np.broadcast_to((i - cy) / fy, (h, w))
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    xy2 = (2.0 * x) * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    return fx * xd + cx, fy * yd + cy


def fixed_point(u, v):
    """iu, iv = rint(u * 32), rint(v * 32) (ties to even) as int32 after saturation."""
    lo, hi = -2147483648.0, 2147483647.0
    return (np.clip(np.rint(u * 32.0), lo, hi).astype(np.int32), np.clip(np.rint(v * 32.0), lo, hi).astype(np.int32))


def make_map(cam, d):
    """The stored map: X (clamped to [-2, w]), Y (clamped to [-2, h]) as int16, ax, ay as uint8 (0..31)."""
    w, h = cam["width"], cam["height"]
    iu, iv = fixed_point(*raw_uv(cam, d))
    X = np.clip(iu >> 5, -2, w).astype(np.int16)
    Y = np.clip(iv >> 5, -2, h).astype(np.int16)
    return X, Y, (iu & 31).astype(np.uint8), (iv & 31).astype(np.uint8)


def remap(img, X, Y, ax, ay):
    """out = ((32-ax)(32-ay) p00 + ax (32-ay) p01 + (32-ax) ay p10 + ax ay p11 + 512) >> 10, taps outside = 0."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    pad = np.zeros((h + 4, w + 4), np.int64)  # rows -2 .. h+1, columns -2 .. w+1
    pad[2:h + 2, 2:w + 2] = img
    Xi, Yi = X.astype(np.int64) + 2, Y.astype(np.int64) + 2
    a, b = ax.astype(np.int64), ay.astype(np.int64)
    p00, p01 = pad[Yi, Xi], pad[Yi, Xi + 1]
    p10, p11 = pad[Yi + 1, Xi], pad[Yi + 1, Xi + 1]
    s = (32 - a) * (32 - b) * p00 + a * (32 - b) * p01 + (32 - a) * b * p10 + a * b * p11
    return ((s + 512) >> 10).astype(np.uint8)


def undistort(img, cam, d):
    return remap(img, *make_map(cam, d))


def pack_frac(ax, ay):
    """The CV_16UC1 half of the downloaded map: (ay << 5) | ax."""
    return (ay.astype(np.uint16) << 5) | ax.astype(np.uint16)


def raw_pixel(cam, d, p):
    """(u, v) of the contract for one undistorted pixel p = (j, i): Python floats, the contract's order."""
    fx, fy, cx, cy = float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])
    k1, k2, p1, p2, k3 = (float(v) for v in d)
    x = (float(p[0]) - cx) / fx
    y = (float(p[1]) - cy) / fy
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    xy2 = (2.0 * x) * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    return fx * xd + cx, fy * yd + cy


def undistorted_pixel(cam, d, raw, iterations=ITERATIONS):
    """The inverse of raw_pixel: x <- (xd - tangential(x)) / kr(x), `iterations` times from the distorted point."""
    fx, fy, cx, cy = float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])
    k1, k2, p1, p2, k3 = (float(v) for v in d)
    xd = (float(raw[0]) - cx) / fx
    yd = (float(raw[1]) - cy) / fy
    x, y = xd, yd
    for _ in range(iterations):
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = p1 * xy2 + p2 * (r2 + 2.0 * x2)
        dy = p1 * (r2 + 2.0 * y2) + p2 * xy2
        x = (xd - dx) / kr
        y = (yd - dy) / kr
    return fx * x + cx, fy * y + cy


def undistorted_pixels(cam, d, raw, iterations=ITERATIONS):
    """undistorted_pixel over an (..., 2) array (the same operations elementwise, so the same bits)."""
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2, k3 = (np.float64(v) for v in d)
    raw = np.asarray(raw, np.float64)
    xd = (raw[..., 0] - cx) / fx
    yd = (raw[..., 1] - cy) / fy
    x, y = xd, yd
    for _ in range(iterations):
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dx = p1 * xy2 + p2 * (r2 + 2.0 * x2)
        dy = p1 * (r2 + 2.0 * y2) + p2 * xy2
        x = (xd - dx) / kr
        y = (yd - dy) / kr
    return np.stack([fx * x + cx, fy * y + cy], axis=-1)


def distort_image(ideal, cam, d):
    """The raw image a lens d would record of the ideal (pinhole) image: raw(p) = ideal(undistorted_pixel(p)), float
    bilinear, 0 outside the ideal image, rounded to bytes.  (Test scenes; not part of the contract.)"""
    h, w = ideal.shape
    grid = np.stack(np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)), axis=-1)
    # (at a raw border that sees past the lens model's monotone range the iteration may diverge: such a point is outside)
    q = np.nan_to_num(undistorted_pixels(cam, d, grid), nan=-1e9, posinf=1e9, neginf=-1e9)
    x0, y0 = np.floor(q[..., 0]), np.floor(q[..., 1])
    a, b = q[..., 0] - x0, q[..., 1] - y0
    pad = np.zeros((h + 2, w + 2))
    pad[1:h + 1, 1:w + 1] = ideal
    xi = np.clip(x0, -1, w - 1).astype(np.int64) + 1
    yi = np.clip(y0, -1, h - 1).astype(np.int64) + 1
    inside = (x0 >= -1) & (x0 < w) & (y0 >= -1) & (y0 < h)
    v = ((1 - a) * (1 - b) * pad[yi, xi] + a * (1 - b) * pad[yi, xi + 1] + (1 - a) * b * pad[yi + 1, xi] +
         a * b * pad[yi + 1, xi + 1])
    return np.where(inside, np.clip(np.rint(v), 0, 255), 0).astype(np.uint8)
