"""Python mirror of the reference's class surface for the alignment hot path, over the C ABI.

Names, argument meaning and error behaviour follow the reference:
  PinholeCamera      include/pinhole_camera.hpp:16 (the pinhole path on undistorted pixels, src/pinhole_camera.cpp:50-101;
                     distortion is removed from the image once, ahead of the pyramid: undistort_image)
  ImagePyramid       include/image_pyramid.hpp:23-149          (device resident; getters download)
  Frame / Feature / Point   include/frame.hpp:70-208, include/feature.hpp:14, include/point.hpp:14
  ImageAlignment     include/image_alignment.hpp:15-73         (align(ref, cur) -> error, cur pose in place)
  FeatureAlignment   include/feature_alignment.hpp:15-43       (align(feature, cur, px) -> error, px in place)
plus the batched forms the GPU is built for (AlignBatch, FeatureAlignment.align_batch).
"""
import ctypes
import math
import operator
import time

import numpy as np

from . import _capi
from ._capi import check, lib, ptr

_default_ctx = {}


class Context:
    """One HIP stream on one GPU (svo_ctx)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib().svo_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)

    @property
    def stream(self):
        return lib().svo_ctx_stream(self.handle)

    def synchronize(self):
        check(lib().svo_ctx_synchronize(self.handle))

    def record(self, slot):
        """hipEventRecord(slot) on this context's stream."""
        check(lib().svo_ctx_event_record(self.handle, int(slot)))

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        check(lib().svo_ctx_event_elapsed(self.handle, int(a), int(b), ctypes.byref(ms)))
        return ms.value

    def close(self):
        if self.handle:
            lib().svo_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def device_count():
    n = ctypes.c_int32()
    check(lib().svo_device_count(ctypes.byref(n)))
    return n.value


UNDISTORT_POINT_ITERATIONS = 40  # include/svo_c.h SVO_UNDISTORT_POINT_ITERATIONS


class UndistortMap:
    """The device-resident fixed-point undistortion map of one camera on one context (svo_undistort_map)."""

    def __init__(self, camera, ctx=None):
        self.ctx = ctx or default_context()
        self.width, self.height = camera.width, camera.height
        h = ctypes.c_void_p()
        cam, d = camera.as_c(), _capi.SvoDistortion(*camera.d)
        check(lib().svo_undistort_map_create(self.ctx.handle, ctypes.byref(cam), ctypes.byref(d), ctypes.byref(h)))
        self.handle = h

    def download(self):
        """(xy (h, w, 2) int16: X, Y; frac (h, w) uint16: ay << 5 | ax), OpenCV's CV_16SC2 + CV_16UC1 pair."""
        xy = np.empty((self.height, self.width, 2), np.int16)
        frac = np.empty((self.height, self.width), np.uint16)
        check(lib().svo_undistort_map_download(self.handle, ptr(xy), ptr(frac)))
        return xy, frac

    def undistort(self, images):
        """PinholeCamera::undistortImage for one (h, w) image or a (count, h, w) stack (svo_undistort_images)."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        if imgs.ndim not in (2, 3) or imgs.shape[-2:] != (self.height, self.width):
            raise ValueError(f"image shape {imgs.shape} does not end in ({self.height}, {self.width})")
        out = np.empty_like(imgs)
        count = imgs.shape[0] if imgs.ndim == 3 else 1
        check(lib().svo_undistort_images(self.ctx.handle, self.handle, ptr(imgs), ptr(out), count))
        return out

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            lib().svo_undistort_map_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinholeCamera:
    """PinholeCamera(width, height, fx, fy, cx, cy, d0..d4) (include/pinhole_camera.hpp:16).  d = (k1, k2, p1, p2, k3)
    in OpenCV's order describes the RAW image; it is consumed once per frame, ahead of the pyramid (undistort_image,
    PyramidSet.upload(camera=...), Frame).  project2d, inverse_project2d, is_in_frame and as_c are the plain pinhole
    and operate on UNDISTORTED pixels, whatever d is: the reference's distorted project2d (src/pinhole_camera.cpp:58-72)
    is wrong upstream and never meets an undistorted image, and is not mirrored.  raw_pixel / undistorted_pixel carry a
    point between the two images."""

    def __init__(self, width, height, fx, fy, cx, cy, d0=0.0, d1=0.0, d2=0.0, d3=0.0, d4=0.0):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.d = (float(d0), float(d1), float(d2), float(d3), float(d4))
        self._maps = {}  # context -> UndistortMap, created on first use

    @classmethod
    def kitti(cls):  # resource/kitti.yaml:7-8, config/config.json:10-11
        return cls(1241, 376, 721.5377, 721.5377, 609.5593, 172.8540)

    @property
    def apply_distortion(self):
        """Any coefficient non-zero (the reference tests |d0| > 1e-5 alone: a deliberate difference, include/svo_c.h)."""
        return any(v != 0.0 for v in self.d)

    def undistort_map(self, ctx=None):
        ctx = ctx or default_context()
        m = self._maps.get(ctx)
        if m is None or not m.handle:
            m = self._maps[ctx] = UndistortMap(self, ctx)
        return m

    def undistort_image(self, img, ctx=None):  # src/pinhole_camera.cpp:178-184 (a copy when nothing applies, :183)
        if not self.apply_distortion:
            return np.array(img, dtype=np.uint8, copy=True)
        return self.undistort_map(ctx).undistort(img)

    def _distort(self, x, y):  # (kr, tangential x, tangential y) at a normalised point
        k1, k2, p1, p2, k3 = self.d
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        return kr, p1 * xy2 + p2 * (r2 + 2.0 * x2), p1 * (r2 + 2.0 * y2) + p2 * xy2

    def raw_pixel(self, p):
        """Where the undistorted pixel p = (j, i) lies in the raw image: the unrounded (u, v) of the map contract."""
        k1, k2, p1, p2, k3 = self.d
        x = (float(p[0]) - self.cx) / self.fx
        y = (float(p[1]) - self.cy) / self.fy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)  # the contract's order, left to right
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
        return np.array([self.fx * xd + self.cx, self.fy * yd + self.cy])

    def undistorted_pixel(self, raw):
        """The inverse of raw_pixel: x <- (xd - tangential(x)) / kr(x), UNDISTORT_POINT_ITERATIONS times from the
        distorted normalised point."""
        xd = (float(raw[0]) - self.cx) / self.fx
        yd = (float(raw[1]) - self.cy) / self.fy
        x, y = xd, yd
        for _ in range(UNDISTORT_POINT_ITERATIONS):
            kr, tx, ty = self._distort(x, y)
            x = (xd - tx) / kr
            y = (yd - ty) / kr
        return np.array([self.fx * x + self.cx, self.fy * y + self.cy])

    def as_c(self):
        return _capi.SvoCamera(self.fx, self.fy, self.cx, self.cy, self.width, self.height)

    def as_dict(self):
        return dict(fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, width=self.width, height=self.height)

    def project2d(self, p):  # src/pinhole_camera.cpp:53-57
        return np.array([self.fx * (p[0] / p[2]) + self.cx, self.fy * (p[1] / p[2]) + self.cy])

    def inverse_project2d(self, px):  # src/pinhole_camera.cpp:84-100
        v = np.array([(px[0] - self.cx) / self.fx, (px[1] - self.cy) / self.fy, 1.0])
        return v * (1.0 / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))

    def is_in_frame(self, p, boundary=0.0):  # src/pinhole_camera.cpp:163-168
        return p[0] >= boundary and p[1] >= boundary and p[0] < self.width - boundary and p[1] < self.height - boundary


def _pixel_format(pixel_format):
    if pixel_format not in _capi.PIXEL_FORMATS:
        raise ValueError(f"unknown pixel format {pixel_format!r}: one of {', '.join(_capi.PIXEL_FORMATS)}")
    return _capi.PIXEL_FORMATS[pixel_format]


def _image_layout(images, pixel_format, gray16_shift, height, width):
    """(array, count, svo_image_layout) of one image or a stack in a pixel format (include/svo_c.h, "pixel formats").
    The format is never guessed: shape and dtype must fit it (ValueError).  A view whose pixels are contiguous and
    whose rows and images lie at non-negative strides that clear a row / an image is passed with its strides; anything
    else is made contiguous first."""
    fmt = _pixel_format(pixel_format)
    bpp, dtype, channels = _capi.PIXEL_SHAPES[pixel_format]
    a = np.asarray(images)
    if a.dtype != np.dtype(dtype):
        raise ValueError(f"pixel format {pixel_format!r} takes {dtype} images, not {a.dtype}")
    want = (height, width, channels) if channels else (height, width)
    if a.ndim not in (len(want), len(want) + 1) or a.shape[a.ndim - len(want):] != want:
        raise ValueError(f"image shape {a.shape} does not fit pixel format {pixel_format!r}: "
                         f"{want} or (count,) + {want}")
    stacked = a.ndim == len(want) + 1
    count = a.shape[0] if stacked else 1
    item = a.dtype.itemsize
    row_bytes = width * bpp
    row = a.strides[-len(want)] if height > 1 else row_bytes
    image = a.strides[0] if stacked and count > 1 else row * height
    pixels_ok = a.flags.aligned and a.strides[-1] == item and (not channels or a.strides[-2] == bpp)
    if not (pixels_ok and row >= row_bytes and image >= row * (height - 1) + row_bytes):
        a = np.require(a, requirements=["C", "A"])  # contiguous and aligned
        row, image = row_bytes, row_bytes * height
    return a, count, _capi.SvoImageLayout(fmt, int(gray16_shift), row, image)


def convert_images(images, pixel_format, gray16_shift=8, ctx=None):
    """The grey image(s) of one (h, w[, channels]) image or a stack in a pixel format, on the device, host to host
    (svo_convert_images)."""
    a = np.asarray(images)
    channels = _capi.PIXEL_SHAPES[pixel_format][2] if pixel_format in _capi.PIXEL_FORMATS else 0
    base = 3 if channels else 2
    if a.ndim not in (base, base + 1):
        raise ValueError(f"image shape {a.shape} does not fit pixel format {pixel_format!r}")
    height, width = a.shape[a.ndim - base], a.shape[a.ndim - base + 1]
    a, count, layout = _image_layout(a, pixel_format, gray16_shift, height, width)
    out = np.empty(((count,) if a.ndim == base + 1 else ()) + (height, width), np.uint8)
    ctx = ctx or default_context()
    check(lib().svo_convert_images(ctx.handle, ctypes.byref(layout), width, height, count, ptr(a), ptr(out)))
    return out


class PyramidSet:
    """n_frames device-resident (image, gradient) stacks of equal geometry (svo_pyramid_set)."""

    def __init__(self, n_frames, width, height, levels, ctx=None):
        self.ctx = ctx or default_context()
        self.n_frames, self.width, self.height, self.levels = int(n_frames), int(width), int(height), int(levels)
        h = ctypes.c_void_p()
        check(lib().svo_pyramid_set_create(self.ctx.handle, self.n_frames, self.width, self.height, self.levels,
                                           ctypes.byref(h)))
        self.handle = h

    def _map_handle(self, camera):
        return camera.undistort_map(self.ctx).handle if camera is not None and camera.apply_distortion else None

    def upload(self, first, images, camera=None, pixel_format="gray8", gray16_shift=8):
        """Level 0 of frames [first, first + count).  With a camera that applies distortion the images are RAW: they
        are undistorted on the device on their way in (svo_pyramid_set_upload_undistort).  pixel_format other than
        "gray8": (h, w, 3 or 4) uint8 colour or (h, w) uint16 images, or stacks of them, converted to grey on the
        device ahead of that (svo_pyramid_set_upload_format; gray16_shift: Y = min(255, v >> shift))."""
        if _pixel_format(pixel_format) != 0:
            imgs, count, layout = _image_layout(images, pixel_format, gray16_shift, self.height, self.width)
            check(lib().svo_pyramid_set_upload_format(self.handle, int(first), count, ptr(imgs), ctypes.byref(layout),
                                                      self._map_handle(camera)))
            self.ctx.synchronize()  # the host buffer may die after return
            return
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        count = imgs.shape[0] if imgs.ndim == 3 else 1
        if imgs.shape[-2:] != (self.height, self.width):
            raise ValueError(f"image shape {imgs.shape[-2:]} != ({self.height}, {self.width})")
        if camera is not None and camera.apply_distortion:
            check(lib().svo_pyramid_set_upload_undistort(self.handle, int(first), count, ptr(imgs),
                                                         camera.undistort_map(self.ctx).handle))
        else:
            check(lib().svo_pyramid_set_upload(self.handle, int(first), count, ptr(imgs)))
        self.ctx.synchronize()  # the host buffer may die after return

    def upload_device(self, first, count, dev_ptr, camera=None, pixel_format="gray8", gray16_shift=8, row_stride=0,
                      image_stride=0):
        """upload() from device memory (count tightly packed images at the address dev_ptr), stream-ordered: the
        memory must stay untouched until the context stream has passed the copy (svo_pyramid_set_upload_device, or
        svo_pyramid_set_upload_undistort_device with a camera that applies distortion).  With a pixel_format other
        than "gray8", or strides in bytes (0: packed), svo_pyramid_set_upload_format_device."""
        src = ctypes.c_void_p(int(dev_ptr))
        fmt = _pixel_format(pixel_format)
        if fmt != 0 or row_stride or image_stride:
            layout = _capi.SvoImageLayout(fmt, int(gray16_shift), int(row_stride), int(image_stride))
            check(lib().svo_pyramid_set_upload_format_device(self.handle, int(first), int(count), src,
                                                             ctypes.byref(layout), self._map_handle(camera)))
            return
        if camera is not None and camera.apply_distortion:
            check(lib().svo_pyramid_set_upload_undistort_device(self.handle, int(first), int(count), src,
                                                                camera.undistort_map(self.ctx).handle))
        else:
            check(lib().svo_pyramid_set_upload_device(self.handle, int(first), int(count), src))

    def build(self, first=0, count=None):
        count = self.n_frames - first if count is None else count
        check(lib().svo_pyramid_set_build(self.handle, int(first), int(count)))

    def build_async(self, first=0, count=None):
        """build() on the context's prep stream, overlapping work queued after it (svo_pyramid_set_build_async):
        every later use of the set through the library waits for it."""
        count = self.n_frames - first if count is None else count
        check(lib().svo_pyramid_set_build_async(self.handle, int(first), int(count)))

    def level_size(self, level):
        w, h = ctypes.c_int32(), ctypes.c_int32()
        check(lib().svo_pyramid_level_size(self.handle, int(level), ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def download(self, frame, level, gradient=False):
        w, h = self.level_size(level)
        out = np.empty((h, w), np.uint8)
        check(lib().svo_pyramid_set_download(self.handle, int(frame), int(level), 1 if gradient else 0, ptr(out)))
        return out

    def close(self):
        # only while the owning context lives: objects kept alive by reference cycles (Frame <-> Feature)
        # may be finalized after their context at interpreter exit
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            lib().svo_pyramid_set_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImagePyramid:
    """ImagePyramid(baseImage, maxPyramidLevel) — device resident (src/image_pyramid.cpp:14-52)."""

    def __init__(self, base_image=None, levels=4, ctx=None, camera=None, pixel_format="gray8", gray16_shift=8):
        self.ctx = ctx or default_context()
        self.levels = int(levels)
        self.set = None
        if base_image is not None:
            self.create_image_pyramid(base_image, levels, camera, pixel_format, gray16_shift)

    def create_image_pyramid(self, base_image, levels, camera=None, pixel_format="gray8", gray16_shift=8):
        """camera: when it applies distortion, base_image is the raw image (PyramidSet.upload).  pixel_format: what
        base_image holds, (h, w) grey or (h, w, channels) colour; level 0 is its grey image (PyramidSet.upload)."""
        if _pixel_format(pixel_format) != 0:
            img = np.asarray(base_image)
            if img.ndim != (3 if _capi.PIXEL_SHAPES[pixel_format][2] else 2):
                raise ValueError(f"ImagePyramid expects one {pixel_format} image, not an array of shape {img.shape}")
            _image_layout(img, pixel_format, gray16_shift, img.shape[0], img.shape[1])  # (before anything is allocated)
            self.levels = int(levels)
            self.set = PyramidSet(1, img.shape[1], img.shape[0], self.levels, self.ctx)
            self.set.upload(0, img, camera, pixel_format, gray16_shift)
            self.set.build(0, 1)
            return
        img = np.ascontiguousarray(base_image, dtype=np.uint8)
        if img.ndim != 2:
            raise ValueError("ImagePyramid expects one 8-bit grey image")
        self.levels = int(levels)
        self.set = PyramidSet(1, img.shape[1], img.shape[0], self.levels, self.ctx)
        self.set.upload(0, img[None], camera)
        self.set.build(0, 1)

    def get_size_image_pyramid(self):
        return 0 if self.set is None else self.levels

    def get_image_at_level(self, level):
        return self.set.download(0, level, False)

    def get_gradient_at_level(self, level):
        return self.set.download(0, level, True)

    def get_base_image(self):
        return self.get_image_at_level(0)

    def get_base_gradient_image(self):
        return self.get_gradient_at_level(0)

    def get_image_size_at_level(self, level):
        if self.set is None or level >= self.levels:
            return (0, 0)
        return self.set.level_size(level)

    def get_base_image_size(self):
        return self.get_image_size_at_level(0)

    def clear(self):
        if self.set is not None:
            self.set.close()
        self.set = None


def _frozen(v):
    """A read-only float64 copy of v (the per-frame SoA caches rely on positions changing only by assignment)."""
    a = np.array(v, dtype=np.float64)
    a.flags.writeable = False
    return a


# Poses are Sophus::SE3d::params(): qx qy qz qw tx ty tz.  The small per-frame pose algebra of System stays on the host.
def _quat_rotate(q, v):
    """q v q^-1 for a unit quaternion (x, y, z, w) and v (3,) or (n, 3), as Eigen's _transformVector forms it."""
    u = np.cross(q[:3], v)
    u = u + u
    return v + q[3] * u + np.cross(q[:3], u)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _norm3(d):
    """|d| with the sum in a fixed order (the C++ mirror forms the same bits)."""
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def pose_inverse(p):
    """Sophus::SE3d::inverse() on params."""
    p = np.asarray(p, np.float64)
    qi = p[:4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([qi, -_quat_rotate(qi, p[4:])])


def pose_compose(a, b):
    """Sophus::SE3d a * b on params (the product quaternion renormalised)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = _quat_mul(a[:4], b[:4])
    q = q / math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.concatenate([q, a[4:] + _quat_rotate(a[:4], b[4:])])


class PointType:  # Point::PointType (include/point.hpp:18-24)
    GOOD, DELETED, CANDIDATE, UNKNOWN = 0, 1, 2, 3


class _PointTable:
    """The state of every live Point as arrays (position, type, m_lastProjectedKFId, the projection counters), one
    row per point: Map.reproject_map gathers these fields of ~2000 points and writes the projection ids back as
    array operations instead of walking the objects.  Rows of collected points are reused."""

    def __init__(self, cap=4096):
        self.pos = np.zeros((cap, 3))
        self.type = np.zeros(cap, np.uint32)
        self.last = np.zeros(cap, np.uint64)
        self.succ = np.zeros(cap, np.int64)
        self.fail = np.zeros(cap, np.int64)
        self.n = 0
        self.free = []

    def alloc(self):
        if self.free:
            return self.free.pop()
        if self.n == len(self.type):
            for k in ("pos", "type", "last", "succ", "fail"):
                a = getattr(self, k)
                b = np.zeros((2 * len(a),) + a.shape[1:], a.dtype)
                b[:len(a)] = a
                setattr(self, k, b)
        self.n += 1
        return self.n - 1


_PT = _PointTable()


class Point:
    """Point(position) (src/point.cpp:6-18): position, type, the observing features and the
    reprojection bookkeeping the Map reads (include/point.hpp:28-40).  The fields live in a row of _PT."""
    NO_FRAME = 2 ** 64 - 1  # m_lastProjectedKFId(-1) on a uint64

    def __init__(self, position):
        i = _PT.alloc()
        self._i = i
        _PT.pos[i] = np.asarray(position, np.float64).reshape(3)  # (a new point is in no frame's cached arrays yet)
        _PT.type[i] = PointType.UNKNOWN
        _PT.last[i] = Point.NO_FRAME
        _PT.succ[i] = 0
        _PT.fail[i] = 0
        self.features = []

    def __del__(self):
        try:
            _PT.free.append(self._i)
        except Exception:  # (interpreter shutdown)
            pass

    # copies own a fresh row: copying _i would alias one row between two Points and put it on the free list twice
    # 
    def _state(self):
        i = self._i
        return (_PT.pos[i].copy(), int(_PT.type[i]), int(_PT.last[i]), int(_PT.succ[i]), int(_PT.fail[i]))

    def __copy__(self):
        return _point_from_state(self._state(), self.features)

    def __deepcopy__(self, memo):
        import copy
        p = _point_from_state(self._state(), ())
        memo[id(self)] = p
        p.features = copy.deepcopy(self.features, memo)
        return p

    def __reduce__(self):
        return (_point_from_state, (self._state(), self.features))

    type = property(lambda self: int(_PT.type[self._i]), lambda self, v: _PT.type.__setitem__(self._i, v))
    last_projected_kf_id = property(lambda self: int(_PT.last[self._i]),
                                    lambda self, v: _PT.last.__setitem__(self._i, v))
    succeeded_projection = property(lambda self: int(_PT.succ[self._i]),
                                    lambda self, v: _PT.succ.__setitem__(self._i, v))
    failed_projection = property(lambda self: int(_PT.fail[self._i]), lambda self, v: _PT.fail.__setitem__(self._i, v))

    def add_feature(self, feature):  # src/point.cpp:35-38
        self.features.append(feature)

    def find_frame(self, frame):  # src/point.cpp: any observing feature in `frame`
        return any(f.frame is frame for f in self.features)

    def remove_frame(self, frame):  # src/point.cpp:40-49: every observing feature that lies in `frame`
        self.features = [f for f in self.features if f.frame is not frame]

    def number_observation(self):  # src/point.cpp:113-116
        return len(self.features)

    # a read-only float64 copy of the row (an in-place edit would not reach the table, so it raises instead).
    # Assigning it bumps a global version that invalidates every Frame's cached point array (a point is not told
    # which frames' features hold it).
    _ver = 0

    @property
    def position(self):
        return _frozen(_PT.pos[self._i])

    @position.setter
    def position(self, v):
        _PT.pos[self._i] = np.asarray(v, np.float64).reshape(3)
        Point._ver += 1


def _point_from_state(state, features):
    """A Point on a row of its own holding `state` (Point._state()) and observed by `features` (copy / pickle)."""
    p = Point(state[0])
    i = p._i
    _PT.type[i], _PT.last[i], _PT.succ[i], _PT.fail[i] = state[1:]
    p.features = list(features)
    return p


class Feature:
    """Feature(frame, pixelPosition, level) — bearing from the frame's camera (src/feature.cpp:14)."""

    # Feature::FeatureType (include/feature.hpp:19-23)
    EDGE, CORNER = 0, 1

    def __init__(self, frame, pixel_position, level=0, point=None, bearing=None, gradient_magnitude=1.0,
                 gradient_orientation=0.0, feature_type=EDGE):
        self._frame = frame
        self._px = _frozen(pixel_position)
        self.level = level
        self.gradient_magnitude = gradient_magnitude      # m_gradientMagnitude (src/feature.cpp:15,34)
        self.gradient_orientation = gradient_orientation  # m_gradientOrientation
        self.type = feature_type
        self._bearing = None if bearing is None else np.asarray(bearing, np.float64)
        self._point = point
        self._pi = -1 if point is None else point._i  # the point's _PT row (-1: none), read by the array gathers
        self._touch()

    @classmethod
    def _many(cls, frame, px, level=0, points=None, gradient_magnitude=None, feature_type=EDGE):
        """Features at the rows of px (n, 2) on `frame` without the per-object property path (the Map and
        FeatureSelection surfaces create hundreds per call): each pixel position is a read-only row of one frozen
        copy of px, points / gradient magnitudes per feature (None: none / 1.0).  Not added to the frame."""
        pxf = _frozen(px)
        n = len(pxf)
        pts = points if points is not None else [None] * n
        gm = gradient_magnitude if gradient_magnitude is not None else [1.0] * n
        out = []
        new = object.__new__
        for i in range(n):
            f = new(cls)
            p = pts[i]
            f.__dict__ = {"_frame": frame, "_px": pxf[i], "level": level, "gradient_magnitude": gm[i],
                          "gradient_orientation": 0.0, "type": feature_type, "_bearing": None, "_point": p,
                          "_pi": -1 if p is None else p._i}
            out.append(f)
        return out

    def _touch(self):  # the owning frame's cached feature arrays are stale
        fr = getattr(self, "_frame", None)
        cell = getattr(fr, "_feat_ver", None)
        if cell is not None:
            cell[0] += 1

    @property
    def frame(self):
        return self._frame

    @frame.setter
    def frame(self, fr):  # both the old and the new frame's cached arrays are stale
        self._touch()
        self._frame = fr
        self._touch()

    # always a read-only float64 array (_feature_arrays joins the raw bytes); assignments invalidate the frame's
    # cached arrays, in-place edits raise (they would leave the cache stale)
    @property
    def pixel_position(self):
        return self._px

    @pixel_position.setter
    def pixel_position(self, v):
        self._px = _frozen(v)
        self._touch()

    @property
    def point(self):
        return self._point

    @point.setter
    def point(self, p):
        self._point = p
        self._pi = -1 if p is None else p._i
        self._touch()

    @property
    def bearing_vec(self):  # formed on first use (the map creates many features that never need it)
        if self._bearing is None:
            self._bearing = np.asarray(self.frame.camera.inverse_project2d(self._px), dtype=np.float64)
        return self._bearing

    def set_point(self, point):
        self.point = point


class _FeatureList(list):
    """Frame.features: a list whose mutations bump the frame's feature version (the cached SoA arrays of
    _feature_arrays are rebuilt only after a change)."""
    __slots__ = ("_cell",)

    def __init__(self, items=(), cell=None):
        super().__init__(items)
        self._cell = cell

    def _bump(self):
        if self._cell is not None:
            self._cell[0] += 1


def _mutator(name):
    base = getattr(list, name)

    def f(self, *a, **k):
        r = base(self, *a, **k)
        self._bump()
        return r if name != "__iadd__" else self
    f.__name__ = name
    return f


for _m in ("append", "extend", "insert", "remove", "pop", "clear", "sort", "reverse", "__setitem__", "__delitem__",
           "__iadd__", "__imul__"):
    setattr(_FeatureList, _m, _mutator(_m))


class Frame:
    """Frame(camera, img, maxImagePyramid, timestamp, lastKeyframe) (src/frame.cpp:6-27).  With a camera that applies
    distortion img is the RAW image; the pyramid holds the undistorted one, and every pixel the frame's features carry
    is an undistorted pixel."""

    _frame_counter = 0  # Frame::m_frameCounter

    def __init__(self, camera, image, max_image_pyramid, timestamp=0, last_keyframe=None, ctx=None,
                 pixel_format="gray8", gray16_shift=8):
        img = np.asarray(image)
        if _pixel_format(pixel_format) != 0:  # colour or 16-bit: the pyramid's level 0 is the frame's grey image
            if img.ndim != (3 if _capi.PIXEL_SHAPES[pixel_format][2] else 2):
                raise ValueError(f"Frame expects one {pixel_format} image, not an array of shape {img.shape}")
            _image_layout(img, pixel_format, gray16_shift, camera.height, camera.width)
        elif img.dtype != np.uint8 or img.ndim != 2 or img.shape != (camera.height, camera.width):
            raise RuntimeError("Image Corrupted")  # src/frame.cpp:20-24
        self.camera = camera
        self.abs_pose = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)  # identity (src/frame.cpp:13)
        self.image_pyramid = ImagePyramid(img, max_image_pyramid, ctx, camera, pixel_format, gray16_shift)
        self._feat_ver = [0]  # bumped by any change to the features (list or Feature attributes)
        self._soa = None      # (key, px, bearing, point, has_point) of the current features
        self.features = []
        self.last_keyframe = last_keyframe
        self.timestamp = timestamp
        self.key_frame = False  # m_keyFrame
        self.id = Frame._frame_counter
        Frame._frame_counter += 1

    def set_keyframe(self):  # src/frame.cpp:29-32
        self.key_frame = True

    def is_keyframe(self):  # src/frame.cpp:78-81
        return self.key_frame

    def number_observation_with_points(self):  # src/frame.cpp:56-67
        return int(np.count_nonzero(_point_rows(self.features) >= 0))

    def world2camera(self, point):  # src/frame.cpp:89-92
        q, t = self.abs_pose[:4], self.abs_pose[4:]
        return _quat_rotate(q, np.asarray(point, np.float64)) + t

    def camera_in_world(self):  # src/frame.cpp:116-120: C = -R^T t
        q = self.abs_pose[:4] * np.array([-1.0, -1.0, -1.0, 1.0])
        return -_quat_rotate(q, self.abs_pose[4:])

    def is_visible(self, point):  # src/frame.cpp:69-76
        pc = self.world2camera(point)
        if pc[2] < 0.0:
            return False
        return bool(self.camera.is_in_frame(self.camera.project2d(pc)))

    def world2image(self, points):
        """Frame::world2image (src/frame.cpp:83-92) for an (n, 3) array (or one point)."""
        pts = np.ascontiguousarray(np.atleast_2d(points), dtype=np.float64)
        out = np.zeros((pts.shape[0], 2))
        cam = self.camera.as_c()
        check(lib().svo_world2image(ctypes.byref(cam), ptr(np.ascontiguousarray(self.abs_pose, np.float64)),
                                    pts.shape[0], ptr(pts), ptr(out)))
        return out if np.ndim(points) == 2 else out[0]

    @property
    def features(self):
        return self._features

    @features.setter
    def features(self, v):
        self._features = _FeatureList(v, self._feat_ver)
        self._feat_ver[0] += 1

    def add_feature(self, feature):
        self.features.append(feature)

    def remove_feature(self, feature):  # src/frame.cpp:39-49 (one bump of the feature version)
        self.features = [f for f in self.features if f is not feature]

    def number_observation(self):
        return len(self.features)

    def feature_arrays(self):
        """This frame's features as SoA arrays (px, bearing, point, has_point), cached until the features change
        (list mutations, Feature.pixel_position / point assignments, any Point.position assignment)."""
        key = (self._feat_ver[0], Point._ver)
        c = self._soa
        if c is None or c[0] != key:
            if c is not None and c[0][0] == key[0]:  # only point positions moved: regather them (same rows)
                self._soa = (key, c[1], c[2], _gather_points(c[5]), c[4], c[5])
            else:
                self._soa = (key, *_feature_soa(self.features))
        return self._soa[1:5]


def _rows(vals, width):
    """float64 arrays of `width` values each -> an (n, width) array.  One join of their raw bytes is ~2x faster
    than np.array over the list (the per-frame gather of ~2000 features is most of align()'s host time).  Feature
    and Point keep these attributes float64 arrays (their setters convert); a duck-typed feature's rows that are
    not all float64 arrays of `width` values (checked per row and by the total length) take np.array's
    conversion."""
    n = len(vals)
    try:
        buf = b"".join([v.tobytes() for v in vals])
        if len(buf) == 8 * width * n and all(v.dtype == np.float64 for v in vals):
            return np.frombuffer(buf, dtype=np.float64).reshape(n, width)
    except AttributeError:
        pass
    return np.array(vals, dtype=np.float64).reshape(n, width)


_get_pi = operator.attrgetter("_pi")


def _point_rows(feats):
    """The _PT rows of the features' points (-1: no point).  A live point's row is never reused (the feature
    holds the point), so each Feature keeps it in _pi."""
    return np.fromiter(map(_get_pi, feats), np.int64, count=len(feats))


def _gather_points(idx):
    out = _PT.pos[np.maximum(idx, 0)]
    out[idx < 0] = 0.0
    return out


def _points_of(feats):
    return _gather_points(_point_rows(feats)) if feats else np.zeros((0, 3))


def _feature_soa(feats):
    """(px, bearing, point, has_point, point rows) of the features."""
    n = len(feats)
    if n == 0:
        return np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.uint8), np.zeros(0, np.int64)
    px = _rows([f.pixel_position for f in feats], 2)
    br = _rows([f.bearing_vec for f in feats], 3)
    idx = _point_rows(feats)
    return px, br, _gather_points(idx), (idx >= 0).astype(np.uint8), idx


def _feature_arrays(frames):
    """The frames' features as SoA arrays (px, bearing, point, has_point), in frame then feature order (each
    frame's arrays cached by Frame.feature_arrays, so a frame that serves as ref or keyframe again costs no
    per-feature gather)."""
    parts = [fr.feature_arrays() for fr in frames]
    if sum(len(p[0]) for p in parts) == 0:
        return np.zeros((1, 2)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros(1, np.uint8)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


MEDIAN_EXACT, MEDIAN_REFERENCE = 0, 1  # include/svo_c.h SVO_MEDIAN_*
REF_MAX_SLOTS = 524288  # include/svo_c.h SVO_REF_MAX_SLOTS


class AlignBatch:
    """n_pairs independent ImageAlignment::align problems on one GPU (svo_align_batch).

    median_mode: MEDIAN_REFERENCE (default) reproduces the reference's robust scale bit for bit (libstdc++
    nth_element post-state, src/algorithm.cpp:834-853); MEDIAN_EXACT uses true order statistics (faster,
    not the reference's numbers: DESIGN.md)."""

    def __init__(self, camera, patch_size, min_level, max_level, n_pairs, max_features, ctx=None,
                 median_mode=MEDIAN_REFERENCE):
        self.ctx = ctx or default_context()
        self.camera = camera
        self.n_pairs = int(n_pairs)
        self.max_level = int(max_level)
        self.median_mode = int(median_mode)
        self._c_cam = camera.as_c()
        self._c_prm = _capi.SvoAlignParams(int(patch_size), int(min_level), int(max_level), self.median_mode)
        h = ctypes.c_void_p()
        check(lib().svo_align_batch_create(self.ctx.handle, ctypes.byref(self._c_cam), ctypes.byref(self._c_prm),
                                           self.n_pairs, int(max_features), ctypes.byref(h)))
        self.handle = h
        self._keep = {}

    def set_pair(self, pair, ref, kf, cur, ref_pose, kf_pose, cur_pose, n_ref, n_kf, px, bearing, point, has_point):
        """ref/kf/cur: (PyramidSet, frame index)."""
        arr = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        px, bearing, point, has_point = arr(px, np.float64), arr(bearing, np.float64), arr(point, np.float64), \
            arr(has_point, np.uint8)
        poses = [arr(p, np.float64) for p in (ref_pose, kf_pose, cur_pose)]
        check(lib().svo_align_batch_set_pair(self.handle, int(pair), ref[0].handle, int(ref[1]), kf[0].handle,
                                             int(kf[1]), cur[0].handle, int(cur[1]), *[ptr(p) for p in poses],
                                             int(n_ref), int(n_kf), ptr(px), ptr(bearing), ptr(point), ptr(has_point)))
        self._keep[pair] = (ref[0], kf[0], cur[0])

    def set_pairs(self, first, ref_set, kf_set, cur_set, frames, poses, n_feat, px, bearing, point, has_point):
        """Bulk set_pair (svo_align_batch_set_pairs) for pairs [first, first + len(frames)): frames (count, 3)
        (ref, kf, cur) indices into the three PyramidSets, poses (count, 3, 7), n_feat (count, 2) = (n_ref,
        n_kf), feature rows packed pair after pair.  Feature arrays may be numpy (host) or CUDA tensors
        (device pointers, copied on the device)."""
        frames = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1, 3)
        count = frames.shape[0]
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(count, 21)
        n_feat = np.ascontiguousarray(n_feat, dtype=np.int32).reshape(count, 2)
        arrs = (px, bearing, point, has_point)
        cuda = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in arrs]
        on_dev = all(cuda)
        if any(cuda) and not on_dev:
            raise ValueError("set_pairs: the feature arrays must be all host arrays or all CUDA tensors")
        if on_dev:
            import torch
            T = int(n_feat.astype(np.int64).sum())
            for name, a, per, dt in (("px", px, 2, (torch.float64,)), ("bearing", bearing, 3, (torch.float64,)),
                                     ("point", point, 3, (torch.float64,)),
                                     ("has_point", has_point, 1, (torch.uint8, torch.int8, torch.bool))):
                if a.dtype not in dt:
                    raise TypeError(f"set_pairs: {name} is {a.dtype}, expected {' / '.join(map(str, dt))}")
                if not a.is_contiguous():
                    raise ValueError(f"set_pairs: {name} must be contiguous")
                if a.device.index != self.ctx.device:
                    raise ValueError(f"set_pairs: {name} is on {a.device}, the batch on cuda:{self.ctx.device}")
                if a.numel() != per * T:
                    raise ValueError(f"set_pairs: {name} has {a.numel()} elements, expected {per} x {T} rows")
            # the scatter runs on the library's streams: whatever torch queued to produce the tensors goes first
            for d in {a.device for a in arrs}:
                torch.cuda.current_stream(d).synchronize()
            ptrs = [ctypes.c_void_p(a.data_ptr()) for a in (px, bearing, point, has_point)]
            keep = (px, bearing, point, has_point)
        else:
            keep = (np.ascontiguousarray(px, dtype=np.float64), np.ascontiguousarray(bearing, dtype=np.float64),
                    np.ascontiguousarray(point, dtype=np.float64), np.ascontiguousarray(has_point, dtype=np.uint8))
            ptrs = [ptr(a) for a in keep]
        check(lib().svo_align_batch_set_pairs(self.handle, int(first), int(count), ref_set.handle, kf_set.handle,
                                              cur_set.handle, ptr(frames), ptr(poses), ptr(n_feat), *ptrs, int(on_dev)))
        for i in range(count):
            self._keep[int(first) + i] = (ref_set, kf_set, cur_set)
        del keep

    def set_initial_poses(self, poses):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.n_pairs, 7)
        check(lib().svo_align_batch_set_initial_poses(self.handle, ptr(poses)))

    def run(self):
        check(lib().svo_align_batch_run(self.handle))

    STAGES = ("init", "residual", "scale", "weights", "solve")

    def profile(self):
        """One synchronous run with events between launches: device ms per stage, summed over levels."""
        ms = (ctypes.c_float * 5)()
        check(lib().svo_align_batch_profile(self.handle, ms))
        return {k: float(v) for k, v in zip(self.STAGES, ms)}

    def results(self):
        poses = np.zeros((self.n_pairs, 7))
        err = np.zeros(self.n_pairs)
        st = np.zeros(self.n_pairs, np.int32)
        check(lib().svo_align_batch_results(self.handle, ptr(poses), ptr(err), ptr(st)))
        return poses, err, st

    def traces(self, pair):
        out = (_capi.SvoLevelTrace * (self.max_level + 1))()
        check(lib().svo_align_batch_traces(self.handle, int(pair), ctypes.cast(out, ctypes.c_void_p)))
        return out

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            lib().svo_align_batch_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImageAlignment:
    """ImageAlignment(patchSize, minLevel, maxLevel, numParameters) (src/image_alignment.cpp:15-67)."""

    def __init__(self, patch_size, min_level, max_level, num_parameters=6, ctx=None, median_mode=MEDIAN_REFERENCE):
        if num_parameters != 6:
            raise ValueError("ImageAlignment estimates SE(3): numParameters must be 6")
        self.patch_size, self.min_level, self.max_level = int(patch_size), int(min_level), int(max_level)
        self.ctx = ctx or default_context()
        self.median_mode = int(median_mode)
        self.last_status = None
        self._traces = None  # the last align()'s per-level traces, fetched on first access (last_traces)
        self._batch = None  # grow-only single-pair batch, reused across align() calls
        self._batch_key = None

    @property
    def last_traces(self):
        """Per-level traces of the last align() (SvoLevelTrace array), or None."""
        if isinstance(self._traces, AlignBatch):
            self._traces = self._traces.traces(0)
        return self._traces

    def align(self, ref_frame, cur_frame):
        """Aligns cur_frame.abs_pose in place; returns the finest level's RMSE (0 if ref has no features)."""
        self._traces = None
        if ref_frame.number_observation() == 0:
            return 0.0
        kf = ref_frame.last_keyframe
        if kf is None:
            raise ValueError("ref_frame.last_keyframe is required (src/image_alignment.cpp:30-31)")
        px, br, pt, hp = _feature_arrays([ref_frame, kf])
        nf = ref_frame.number_observation() + kf.number_observation()
        cam = ref_frame.camera
        key = (cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
        if self._batch is None or self._batch_key != key or self._batch_cap < nf:
            if self._batch is not None:
                self._batch.close()
            grow = 1 if self._batch is None else 2 * self._batch_cap
            if self.median_mode == MEDIAN_REFERENCE:  # doubling must not cross the reference-mode limit
                grow = min(grow, REF_MAX_SLOTS // (self.patch_size * self.patch_size))
            cap = max(nf, grow)
            self._batch = AlignBatch(cam, self.patch_size, self.min_level, self.max_level, 1, cap, self.ctx,
                                     median_mode=self.median_mode)
            self._batch_key, self._batch_cap = key, cap
        b = self._batch
        s = lambda fr: (fr.image_pyramid.set, 0)
        b.set_pair(0, s(ref_frame), s(kf), s(cur_frame), ref_frame.abs_pose, kf.abs_pose, cur_frame.abs_pose,
                   ref_frame.number_observation(), kf.number_observation(), px, br, pt, hp)
        b.run()
        poses, err, st = b.results()
        self._traces = b  # (a device read only when someone asks: not on the per-frame path)
        cur_frame.abs_pose[:] = poses[0]
        self.last_status = int(st[0])
        return float(err[0])


class FeatureAlignment:
    """FeatureAlignment(patchSize, level, numParameters) (src/feature_alignment.cpp:15-62)."""

    def __init__(self, patch_size, level=0, num_parameters=3, ctx=None):
        if num_parameters != 3:
            raise ValueError("FeatureAlignment estimates (u, v, bias): numParameters must be 3")
        self.patch_size, self.level = int(patch_size), int(level)
        self.ctx = ctx or default_context()
        self.last_status = None

    def align(self, ref_feature, cur_frame, pixel_pos):
        """pixel_pos (numpy float64[2]) is updated in place; returns the RMSE (NaN if out of frame)."""
        px = np.ascontiguousarray(pixel_pos, dtype=np.float64).reshape(1, 2).copy()
        err, st = self.align_batch(ref_feature.frame.image_pyramid.set, [0], cur_frame.image_pyramid.set, 0,
                                   ref_feature.pixel_position.reshape(1, 2), px, cur_frame.camera)
        pixel_pos[0], pixel_pos[1] = px[0, 0], px[0, 1]
        self.last_status = int(st[0])
        return float(err[0])

    def align_batch(self, ref_set, ref_frames, cur_set, cur_frame, ref_px, px_inout, camera):
        ref_px = np.ascontiguousarray(ref_px, dtype=np.float64)
        n = ref_px.shape[0]
        if px_inout.dtype != np.float64 or not px_inout.flags.c_contiguous or px_inout.shape != (n, 2):
            raise ValueError("px_inout must be a C-contiguous float64 (n, 2) array")
        rf = np.ascontiguousarray(np.broadcast_to(np.asarray(ref_frames, np.int32), (n,)))
        err = np.zeros(n)
        st = np.zeros(n, np.int32)
        cam = camera.as_c()
        check(lib().svo_feature_align(self.ctx.handle, ctypes.byref(cam), self.patch_size, ref_set.handle, ptr(rf), 0,
                                      cur_set.handle, int(cur_frame), n, ptr(ref_px), ptr(px_inout), ptr(err), ptr(st)))
        return err, st


    def align_many(self, ref_features, cur_frame, px_inout):
        """align() for every (ref_features[i], px_inout[i]) against cur_frame in one launch; each
        reference feature reads the gradient of its own frame (svo_feature_align_multi)."""
        n = len(ref_features)
        if px_inout.dtype != np.float64 or not px_inout.flags.c_contiguous or px_inout.shape != (n, 2):
            raise ValueError("px_inout must be a C-contiguous float64 (n, 2) array")
        err = np.zeros(n)
        st = np.zeros(n, np.int32)
        if n == 0:
            return err, st
        sets = (ctypes.c_void_p * n)(*[f.frame.image_pyramid.set.handle.value for f in ref_features])
        frames = np.zeros(n, np.int32)
        ref_px = np.ascontiguousarray([f.pixel_position for f in ref_features], dtype=np.float64)
        cam = cur_frame.camera.as_c()
        check(lib().svo_feature_align_multi(self.ctx.handle, ctypes.byref(cam), self.patch_size, sets, ptr(frames),
                                            cur_frame.image_pyramid.set.handle, 0, n, ptr(ref_px), ptr(px_inout),
                                            ptr(err), ptr(st)))
        return err, st


# ---------------------------------------------------------------- map reprojection
class Map:
    """Map(camera, cellSize) (src/map.cpp:15-19; grid :222-248): the reprojection half of the reference's
    map, reprojectMap (:260-478) with reprojectPoint (:481-492) and reprojectCell (:495-570),
    addNewCandidate (:586-593), addCandidateToFrame (:595-627) and removeMatchedCandidate (:629-634).

    The reference aligns candidates one FeatureAlignment(7, 0, 3) call at a time; here every alignment of
    a call runs in one launch (svo_feature_align_multi) and the decisions are replayed in the reference's
    order: reprojectCell accepts the first non-deleted candidate of a cell whatever its error, so the
    aligned set is fixed before the alignment (svo_map_reproject_plan); addCandidateToFrame aligns every
    candidate whose cell is free and then lets the first match of each cell win.  The cell order is a
    seeded permutation (the reference shuffles it with an unseeded std::random_device, :243-247)."""

    MAX_MATCHES = 150  # :474

    def __init__(self, camera, cell_size, seed=0, ctx=None):
        self.camera = camera
        self.cell_size = int(cell_size)
        self.grid_cols = int(math.ceil(camera.width / self.cell_size))
        self.grid_rows = int(math.ceil(camera.height / self.cell_size))
        n = self.grid_cols * self.grid_rows
        self.cell_orders = np.random.default_rng(seed).permutation(n).astype(np.int32)
        self.cell_visited = np.zeros(n, bool)  # never cleared by the reference (resetGrid :250-258)
        self.matches = 0
        self.trials = 0
        self.candidates = []  # [feature, point, matched]
        self.alignment = FeatureAlignment(7, 0, 3, ctx)
        self.key_frames = []
        self.native_seconds = 0.0  # time inside the C ABI calls (plan, projection, batched alignment)

    def cell_of(self, px):
        return int(px[1]) // self.cell_size * self.grid_cols + int(px[0]) // self.cell_size

    def reset(self):  # src/map.cpp:21-24
        self.key_frames.clear()

    def add_keyframe(self, frame):  # src/map.cpp:112-115
        self.key_frames.append(frame)

    def size_keyframes(self):  # src/map.cpp:218-221
        return len(self.key_frames)

    def get_close_keyframes(self, frame):
        """getCloseKeyframes (src/map.cpp:144-170): the keyframes in reverse order, `frame` itself skipped; a
        keyframe is listed with |frame.t - keyframe.t| (absPose.translation(), not the camera centres) as soon as
        one of its features' points is visible in `frame`.  The reference dereferences m_point unchecked there; a
        feature without a point is passed over here."""
        out = []
        for kf in reversed(self.key_frames):
            if kf is frame:
                continue
            for f in kf.features:
                if f.point is not None and frame.is_visible(f.point.position):
                    out.append((kf, _norm3(frame.abs_pose[4:] - kf.abs_pose[4:])))
                    break
        return out

    def get_closest_keyframe(self, frame):
        """getClosestKeyframe (src/map.cpp:117-142): the first close keyframe with the strictly smallest distance,
        or None."""
        closest, min_distance = None, float("inf")
        for kf, d in self.get_close_keyframes(frame):
            if kf is not frame and d < min_distance:
                min_distance, closest = d, kf
        return closest

    def get_furthest_keyframe(self, pos):
        """getFurthestKeyframe (src/map.cpp:172-184): the first keyframe whose camera centre is strictly furthest
        from pos (None when every distance is 0)."""
        pos = np.asarray(pos, np.float64)
        furthest, max_distance = None, 0.0
        for kf in self.key_frames:
            dist = _norm3(kf.camera_in_world() - pos)
            if dist > max_distance:
                max_distance, furthest = dist, kf
        return furthest

    def remove_frame(self, frame):
        """removeFrame (src/map.cpp:26-61): every feature of the keyframe leaves its point's observer list
        (Point::removeFrame) and loses the point, the frame's features and last keyframe are dropped, the frame
        leaves the keyframe list, and the candidates seeded from it leave too (removeFrameCandidate, :669-675).  A
        point is not deleted here, whatever number of observers it keeps."""
        for i, fr in enumerate(self.key_frames):
            if fr is frame:
                for f in fr.features:
                    if f.point is not None:
                        f.point.remove_frame(f.frame)
                        f.point = None
                break
        else:
            raise ValueError("remove_frame: not a keyframe of this map")  # (the reference erases past the end)
        frame.features.clear()
        frame.last_keyframe = None
        del self.key_frames[i]
        self.candidates = [c for c in self.candidates if c[0].frame is not frame]

    def remove_point(self, point):  # src/map.cpp:76-87
        for feature in point.features:
            feature.frame.remove_feature(feature)
        point.features.clear()
        point.type = PointType.DELETED

    def remove_feature(self, feature):  # src/map.cpp:89-110
        point = feature.point
        if point is None:
            return
        if point.number_observation() <= 2:
            self.remove_point(point)
            # removePoint nulls the shared_ptr it was handed, which is this feature's m_point (:86, :98); the
            # feature is in no frame any more, so no frame's cached arrays hold it
            feature._point, feature._pi = None, -1
            return
        point.remove_frame(feature.frame)
        feature.frame.remove_feature(feature)  # the feature keeps its m_point (:108 is commented out)

    def reproject_map(self, ref_frame, cur_frame, overlap_keyframes):
        if ref_frame.last_keyframe is None:
            raise ValueError("reprojectMap needs refFrame->m_lastKeyframe")
        kfs = [ref_frame, ref_frame.last_keyframe]
        nfs = [len(kf.features) for kf in kfs]
        off = np.cumsum([0] + nfs).astype(np.int32)
        # the distinct points (their _PT rows) in first-seen order and each feature's index among them (-1: none)
        rows = np.concatenate([_point_rows(kf.features) for kf in kfs])
        valid = rows >= 0
        u, first, inv = np.unique(rows[valid], return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")
        prow = u[order]
        rank = np.empty(len(u), np.int32)
        rank[order] = np.arange(len(u), dtype=np.int32)
        feat_point = np.full(max(len(rows), 1), -1, np.int32)
        feat_point[np.nonzero(valid)[0]] = rank[inv.reshape(-1)]
        npt = len(prow)
        pos = np.ascontiguousarray(_PT.pos[prow]) if npt else np.zeros((1, 3))
        ptype = _PT.type[prow] if npt else np.zeros(1, np.uint32)
        plast = _PT.last[prow] if npt else np.zeros(1, np.uint64)
        n_cells = len(self.cell_orders)
        overlap = np.zeros(len(kfs), np.int32)
        sel_feat = np.zeros(n_cells, np.int32)
        sel_cell = np.zeros(n_cells, np.int32)
        sel_px = np.zeros((n_cells, 2))
        n_sel, m, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        cam = self.camera.as_c()
        t0 = time.perf_counter()
        check(lib().svo_map_reproject_plan(ctypes.byref(cam), self.cell_size, n_cells, ptr(self.cell_orders),
                                           ptr(np.ascontiguousarray(cur_frame.abs_pose, np.float64)),
                                           ctypes.c_uint64(cur_frame.id), len(kfs), ptr(off), ptr(feat_point), npt,
                                           ptr(pos), ptr(ptype), ptr(plast), ptr(overlap), ctypes.byref(n_sel),
                                           ptr(sel_feat), ptr(sel_cell), ptr(sel_px), ctypes.byref(m),
                                           ctypes.byref(t)))
        self.native_seconds += time.perf_counter() - t0
        _PT.last[prow] = plast[:npt]
        for k, kf in enumerate(kfs):
            overlap_keyframes.append((kf, int(overlap[k])))
        self.matches, self.trials = m.value, t.value
        ns = n_sel.value
        f0, f1 = kfs[0].features, kfs[1].features
        n0 = nfs[0]
        chosen = [f0[i] if i < n0 else f1[i - n0] for i in sel_feat[:ns].tolist()]
        px = np.ascontiguousarray(sel_px[:ns])
        t0 = time.perf_counter()
        self.alignment.align_many(chosen, cur_frame, px)
        self.native_seconds += time.perf_counter() - t0
        pts = [f._point for f in chosen]
        new = Feature._many(cur_frame, px, 0, points=pts)
        # :558-569 (m_succeededProjection++, UNKNOWN -> GOOD past 10) on the points' rows; a point is planned at most
        # once per call (m_lastProjectedKFId), and the end state would be the same for repeats
        srow = np.fromiter((p._i for p in pts), np.int64, count=ns)
        np.add.at(_PT.succ, srow, 1)
        up = (_PT.type[srow] == PointType.UNKNOWN) & (_PT.succ[srow] > 10)
        _PT.type[srow[up]] = PointType.GOOD
        for point, feature in zip(pts, new):
            point.features.append(feature)
        cur_frame.features.extend(new)
        self.cell_visited[sel_cell[:ns]] = True

    def add_new_candidate(self, feature, point, matched=False):
        point.type = PointType.CANDIDATE
        self.candidates.append([feature, point, matched])

    def add_candidate_to_frame(self, frame):
        if not self.candidates:
            return
        rows = np.fromiter((c[1]._i for c in self.candidates), np.int64, count=len(self.candidates))
        pos = np.ascontiguousarray(_PT.pos[rows])
        t0 = time.perf_counter()
        px0 = frame.world2image(pos)
        self.native_seconds += time.perf_counter() - t0
        w, h = frame.camera.width, frame.camera.height
        # inside the 3-px border (isInFrame(px, 3)), cell not visited yet (:600-606); cell_of truncates like int()
        inside = (px0[:, 0] >= 3) & (px0[:, 1] >= 3) & (px0[:, 0] < w - 3) & (px0[:, 1] < h - 3)
        cell = np.zeros(len(px0), np.int64)
        cell[inside] = (px0[inside, 1].astype(np.int64) // self.cell_size * self.grid_cols
                        + px0[inside, 0].astype(np.int64) // self.cell_size)
        elig = np.nonzero(inside)[0]
        elig = elig[~self.cell_visited[cell[elig]]]
        cells = cell[elig].tolist()
        px = np.ascontiguousarray(px0[elig])
        cands = [self.candidates[i][0] for i in elig.tolist()]
        t0 = time.perf_counter()
        err, _ = self.alignment.align_many(cands, frame, px)
        self.native_seconds += time.perf_counter() - t0
        ok = (err < 50.0).tolist()
        acc = []
        for j, i in enumerate(elig.tolist()):  # the reference's order: a cell taken earlier in this loop is skipped
            if not ok[j] or self.cell_visited[cells[j]]:
                continue
            self.cell_visited[cells[j]] = True
            acc.append((j, i))
        if acc:
            pts = [self.candidates[i][1] for _, i in acc]
            new = Feature._many(frame, px[[j for j, _ in acc]], 0, points=pts)
            frame.features.extend(new)
            for (_, i), point, feature in zip(acc, pts, new):
                feat = self.candidates[i][0]
                point.features.append(feat)
                point.features.append(feature)
                feat.set_point(point)
                self.candidates[i][2] = True
        self.candidates = [c for c in self.candidates if not c[2]]  # removeMatchedCandidate


# ---------------------------------------------------------------- depth filter
DEPTH_SEED = np.dtype([("a", "f8"), ("b", "f8"), ("mu", "f8"), ("sigma", "f8"), ("var", "f8"), ("max_depth", "f8"),
                       ("px", "f8", 2), ("bearing", "f8", 3), ("kf", "i4"), ("valid", "i4")])  # svo_depth_seed


def depth_seeds(px, bearing, depth_mean, depth_min, kf=0):
    """MixedGaussianFilter(feature, depthMean, depthMin) for each feature (src/mixed_gaussian_filter.cpp:7-24)."""
    n = len(px)
    s = np.zeros(n, DEPTH_SEED)
    one = _capi.SvoDepthSeed()
    check(lib().svo_depth_seed_init(float(depth_mean), float(depth_min), ctypes.byref(one)))
    for k in ("a", "b", "mu", "sigma", "var", "max_depth"):
        s[k] = getattr(one, k)
    s["px"], s["bearing"], s["kf"], s["valid"] = px, bearing, kf, 1
    return s


def depth_update(camera, keyframes, cur, cur_pose, seeds, ctx=None):
    """DepthEstimator::updateFilters for `seeds` (DEPTH_SEED array) against the current frame.

    keyframes: list of (PyramidSet, frame index, pose[7]); seed["kf"] indexes it.  cur: (PyramidSet, frame).
    Returns (survivors, outcome[n], cand_points[m, 3], cand_seed[m]) in the reference's orders."""
    ctx = ctx or default_context()
    seeds = np.ascontiguousarray(seeds, DEPTH_SEED).copy()
    n = len(seeds)
    nk = len(keyframes)
    sets = (ctypes.c_void_p * max(nk, 1))(*[k[0].handle.value for k in keyframes])
    frames = np.array([k[1] for k in keyframes] or [0], np.int32)
    poses = np.ascontiguousarray(np.array([k[2] for k in keyframes] or [np.zeros(7)], np.float64))
    cp = np.ascontiguousarray(cur_pose, np.float64)
    outcome = np.zeros(max(n, 1), np.int32)
    pts = np.zeros((max(n, 1), 3))
    cs = np.zeros(max(n, 1), np.int32)
    n_out, n_cand = ctypes.c_int32(), ctypes.c_int32()
    cam = camera.as_c()
    check(lib().svo_depth_update(ctx.handle, ctypes.byref(cam), nk, ctypes.cast(sets, ctypes.c_void_p), ptr(frames),
                                 ptr(poses), cur[0].handle, int(cur[1]), ptr(cp), n, ptr(seeds), ctypes.byref(n_out),
                                 ptr(outcome), ptr(pts), ptr(cs), ctypes.byref(n_cand)))
    return seeds[:n_out.value].copy(), outcome[:n], pts[:n_cand.value].copy(), cs[:n_cand.value].copy()


class DepthEstimator:
    """DepthEstimator (include/depth_estimator.hpp, src/depth_estimator.cpp) without its worker thread:
    add_keyframe = initializeFilters (:175-190) for the keyframe's features without a point,
    update_filters = updateFilters (:192-309).  Converged seeds become candidates (Map::addNewCandidate,
    src/map.cpp:586-593): (feature, Point) pairs in the reference's order."""

    def __init__(self, ctx=None, map=None):
        self.ctx = ctx or default_context()
        self.map = map        # m_map: add_frame hands the converged seeds to it (None: they stay in candidates)
        self.keyframes = []   # Frame objects; seed["kf"] indexes this list
        self.features = []    # the Feature behind every seed, same order as self.seeds
        self.seeds = np.zeros(0, DEPTH_SEED)
        self.candidates = []
        self._deleted_keyframe = None  # m_deletedKeyframe

    def reset(self):  # src/depth_estimator.cpp:99-109
        self.keyframes, self.features, self.seeds = [], [], np.zeros(0, DEPTH_SEED)
        self._deleted_keyframe = None

    def remove_keyframe(self, frame):
        """removeKeyframe (src/depth_estimator.cpp:88-92): the frame is buffered; its seeds leave at the next
        add_frame / add_keyframe (the reference's worker drops them before its next update, :145-148, :161-173)."""
        self._deleted_keyframe = frame

    def _drop_deleted_keyframe(self):
        frame, self._deleted_keyframe = self._deleted_keyframe, None
        if frame is None:
            return
        keep = [i for i, f in enumerate(self.features) if f.frame is not frame]
        self.features = [self.features[i] for i in keep]
        self.seeds = self.seeds[keep].copy() if keep else np.zeros(0, DEPTH_SEED)
        remap = np.full(len(self.keyframes), -1, np.int32)  # the keyframe table without the frame
        kept = [k for k, kf in enumerate(self.keyframes) if kf is not frame]
        remap[kept] = np.arange(len(kept), dtype=np.int32)
        self.keyframes = [self.keyframes[k] for k in kept]
        if len(self.seeds):
            self.seeds["kf"] = remap[self.seeds["kf"]]

    def add_frame(self, frame):
        """addFrame (src/depth_estimator.cpp:50-65), the m_thread == nullptr branch: updateFilters(frame), the
        converged seeds handed to the map (Map::addNewCandidate, :288).  Returns them."""
        self._drop_deleted_keyframe()
        new = self.update_filters(frame)
        if self.map is not None:
            for feature, point in new:
                self.map.add_new_candidate(feature, point)
        return new

    def add_keyframe(self, frame, depth_mean, depth_min):
        self._drop_deleted_keyframe()
        feats = [f for f in frame.features if f.point is None]
        kf = len(self.keyframes)
        self.keyframes.append(frame)
        if feats:
            px = np.array([f.pixel_position for f in feats])
            br = np.array([f.bearing_vec for f in feats])
            self.seeds = np.concatenate([self.seeds, depth_seeds(px, br, depth_mean, depth_min, kf)])
            self.features += feats

    def number_filters(self):
        return len(self.seeds)

    def update_filters(self, frame):
        if len(self.seeds) == 0:
            return []
        kfs = [(k.image_pyramid.set, 0, k.abs_pose) for k in self.keyframes]
        surv, outcome, pts, cs = depth_update(frame.camera, kfs, (frame.image_pyramid.set, 0), frame.abs_pose,
                                              self.seeds, self.ctx)
        new = [(self.features[i], Point(p)) for i, p in zip(cs, pts)]
        self.candidates += new
        keep = [i for i in range(len(self.seeds)) if outcome[i] in (1, 2) and self.seeds[i]["valid"]]  # still seeds
        self.features = [self.features[i] for i in keep]
        self.seeds = surv
        return new


# ---------------------------------------------------------------- feature selection
class FeatureSelection:
    """FeatureSelection(width, height, cellSize) (src/feature_selection.cpp:19-287).

    The occupancy grid ((height // cellSize + 1) x (width // cellSize + 1) cells) lives here on the host
    like the reference's member; detection reads the frame's device-resident level-0 gradient plane."""

    def __init__(self, width, height, cell_size, ctx=None):
        self.ctx = ctx or default_context()
        r, c = ctypes.c_int32(), ctypes.c_int32()
        check(lib().svo_feature_grid_size(int(width), int(height), int(cell_size), ctypes.byref(r), ctypes.byref(c)))
        self.width, self.height, self.cell_size = int(width), int(height), int(cell_size)
        self.grid_rows, self.grid_cols = r.value, c.value
        self.occupancy_grid = np.zeros((self.grid_rows, self.grid_cols), np.uint8)
        self.last_keypoints = 0

    def set_existing_features(self, features):  # :268-274
        for f in features:
            self.set_cell_in_grid_occupancy(f.pixel_position)

    def set_cell_in_grid_occupancy(self, location):  # :276-282 (uint32 truncation of the division)
        self.occupancy_grid[int(location[1] / self.cell_size), int(location[0] / self.cell_size)] = 1

    def reset_grid_occupancy(self):  # :284-287
        self.occupancy_grid[:] = 0

    def _emit(self, frame, px, resp, n):
        frame.features.extend(Feature._many(frame, px[:n], 0, gradient_magnitude=resp[:n].tolist(),
                                            feature_type=Feature.EDGE))
        return n

    def detect(self, frame, detection_threshold):
        """The device step alone: keys (response << 24 | y * width + x) above the threshold, row-major."""
        cap = self.width * self.height
        keys = np.zeros(cap, np.uint32)
        n = ctypes.c_int32()
        check(lib().svo_feature_detect(self.ctx.handle, frame.image_pyramid.set.handle, 0, int(detection_threshold),
                                       cap, ptr(keys), ctypes.byref(n)))
        return keys[:n.value]

    def gradient_magnitude_with_ssc(self, frame, detection_threshold, number_candidate, use_bucketing):
        """:27-89 — adds the selected features to `frame` (EDGE, level 0); returns how many."""
        cap = self.grid_rows * self.grid_cols if use_bucketing else max(4 * int(number_candidate), 1024)
        while True:
            px = np.zeros((cap, 2))
            resp = np.zeros(cap)
            n, nk = ctypes.c_int32(), ctypes.c_int32()
            occ = self.occupancy_grid.copy()
            rc = lib().svo_feature_select_ssc(self.ctx.handle, frame.image_pyramid.set.handle, 0,
                                              int(detection_threshold), int(number_candidate), int(bool(use_bucketing)),
                                              self.cell_size, ptr(occ), cap, ptr(px), ptr(resp), ctypes.byref(n),
                                              ctypes.byref(nk))
            if rc == _capi.SVO_ERR_ARG and not use_bucketing and cap < self.width * self.height:
                cap = self.width * self.height  # SSC kept more than the first guess
                continue
            check(rc)
            break
        self.occupancy_grid[:] = occ
        self.last_keypoints = nk.value
        return self._emit(frame, px, resp, n.value)

    def gradient_magnitude_by_value(self, frame, detection_threshold, use_bucketing=True):
        """:91-143 — bucketing branch (the reference's other branch reads the 8-bit magnitude as float)."""
        if not use_bucketing:
            raise ValueError("gradientMagnitudeByValue without bucketing reads the u8 magnitude as float "
                             "(src/feature_selection.cpp:150); not supported")
        cap = self.grid_rows * self.grid_cols
        px = np.zeros((cap, 2))
        resp = np.zeros(cap)
        n = ctypes.c_int32()
        occ = self.occupancy_grid.copy()
        check(lib().svo_feature_select_by_value(self.ctx.handle, frame.image_pyramid.set.handle, 0,
                                                int(detection_threshold), self.cell_size, ptr(occ), cap, ptr(px),
                                                ptr(resp), ctypes.byref(n)))
        self.occupancy_grid[:] = occ
        return self._emit(frame, px, resp, n.value)


SCALE_AUTO, SCALE_K2R, SCALE_K2V, SCALE_K2 = 0, 1, 2, 3  # include/svo_c.h SVO_SCALE_*


def robust_scale_capacity(impl):
    """Largest residual vector (features x patch^2) the kernel `impl` takes (svo_robust_scale_capacity)."""
    v = ctypes.c_int64()
    check(lib().svo_robust_scale_capacity(int(impl), ctypes.byref(v)))
    return int(v.value)
SCALE_K2V_MAX_SLOTS = 128 * 512             # K2V holds the vector in registers (align_refv.hip LayC)
SCALE_K2V_LAYB_SLOTS = 118 * 512            # (LayB)
SCALE_K2V_LAYA_SLOTS = 98 * 512             # (LayA: the faster layout, the config-2 shape)


def debug_robust_scale(values, n_valid, ctx=None, impl=SCALE_AUTO, diagnostics=False):
    """svo_debug_robust_scale: algorithm::computeMAD(values, n_valid) with the reference's libstdc++
    nth_element post-state (MEDIAN_REFERENCE), on the device with kernel `impl` (SCALE_*); returns (median,
    mad), or (median, mad, diagnostics) with diagnostics=True (the 204 doubles after them, see
    include/svo_c.h).  values: the full residual vector, invisible slots = DBL_MAX (src/optimizer.cpp:387-396)."""
    ctx = ctx or default_context()
    v = np.ascontiguousarray(values, np.float64)
    # without diagnostics only med / mad come back, and K2V runs the product kernel's own code path (svo_c.h)
    out = np.zeros(206 if diagnostics else 2)
    check(lib().svo_debug_robust_scale(ctx.handle, ptr(v), len(v), int(n_valid), int(impl), ptr(out), len(out)))
    if diagnostics:
        return float(out[0]), float(out[1]), out[2:].copy()
    return float(out[0]), float(out[1])


# ---------------------------------------------------------------- pose-only bundle adjustment
def pose_optimize_batch(feat_off, bearing, point, has_point, vis, poses, ctx=None):
    """svo_pose_optimize over arrays: frame f owns rows feat_off[f]:feat_off[f+1].  vis (uint8, in/out) and
    poses ((F, 7), in/out) are updated in place; returns (err, status)."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    F = len(feat_off) - 1
    for a, dt in ((vis, np.uint8), (poses, np.float64)):
        if a.dtype != dt or not a.flags.c_contiguous:
            raise ValueError("vis must be C-contiguous uint8 and poses C-contiguous float64")
    bearing = np.ascontiguousarray(bearing, np.float64)
    point = np.ascontiguousarray(point, np.float64)
    has_point = np.ascontiguousarray(has_point, np.uint8)
    err = np.zeros(F)
    st = np.zeros(F, np.int32)
    check(lib().svo_pose_optimize(ctx.handle, F, ptr(feat_off), ptr(bearing), ptr(point), ptr(has_point), ptr(vis),
                                  ptr(poses), ptr(err), ptr(st)))
    return err, st


class BundleAdjustResult:
    """Outputs of bundle_adjust_batch (include/svo_c.h svo_bundle_adjust): obs_chi2 (n_obs,), init_chi, final_chi,
    iterations, status (n_problems,), trace (n_problems, BA_TRACE_CAP, 6) or None."""
    __slots__ = ("obs_chi2", "init_chi", "final_chi", "iterations", "status", "trace")


BA_MAX_FRAMES = 16  # SVO_BA_MAX_FRAMES: free frames per problem (fixed frames are not limited)
BA_TRACE_CAP = 64   # SVO_BA_TRACE_CAP


def bundle_adjust_batch(camera, frame_off, point_off, obs_off, poses, frame_fixed, points, obs_frame, obs_point,
                        obs_px, huber_delta, max_iterations=10, structure_iterations=0, trace=False, ctx=None):
    """svo_bundle_adjust over arrays: the windowed bundle adjustment of twoViewBA / localBA
    (src/bundle_adjustment.cpp:397-625) for independent problems.  The cost and the Levenberg-Marquardt schedule are
    this project's contract (include/svo_c.h), modelled on g2o's and not pinned to it.  Problem p owns frames
    frame_off[p]:frame_off[p+1], points point_off[p]:..., observations obs_off[p]:... (local indices, grouped by
    point, points ascending).  poses ((n_frames, 7)) and points ((n_points, 3)), float64 and C-contiguous, are
    updated in place."""
    frame_off = np.ascontiguousarray(frame_off, np.int32)
    point_off = np.ascontiguousarray(point_off, np.int32)
    obs_off = np.ascontiguousarray(obs_off, np.int32)
    if not (len(frame_off) == len(point_off) == len(obs_off) >= 1):
        raise ValueError("frame_off, point_off and obs_off must hold n_problems + 1 entries each")
    NP = len(frame_off) - 1
    nf, nx, no = int(frame_off[-1]), int(point_off[-1]), int(obs_off[-1])
    _c_f64(poses, (nf, 7), "poses")
    _c_f64(points, (nx, 3), "points")
    frame_fixed = np.ascontiguousarray(frame_fixed, np.uint8).reshape(nf)
    obs_frame = np.ascontiguousarray(obs_frame, np.int32).reshape(no)
    obs_point = np.ascontiguousarray(obs_point, np.int32).reshape(no)
    obs_px = np.ascontiguousarray(obs_px, np.float64).reshape(no, 2)
    r = BundleAdjustResult()
    r.obs_chi2 = np.zeros(no)
    r.init_chi = np.zeros(NP)
    r.final_chi = np.zeros(NP)
    r.iterations = np.zeros(NP, np.int32)
    r.status = np.zeros(NP, np.int32)
    r.trace = np.zeros((NP, BA_TRACE_CAP, 6)) if trace else None
    cam = camera.as_c()
    ctx = ctx or default_context()
    check(lib().svo_bundle_adjust(ctx.handle, ctypes.byref(cam), NP, ptr(frame_off), ptr(point_off), ptr(obs_off),
                                  ptr(poses), ptr(frame_fixed), ptr(points), ptr(obs_frame), ptr(obs_point),
                                  ptr(obs_px), float(huber_delta), int(max_iterations), int(structure_iterations),
                                  ptr(r.obs_chi2), ptr(r.init_chi), ptr(r.final_chi), ptr(r.iterations),
                                  ptr(r.status), ptr(r.trace) if trace else None))
    return r


class BundleAdjustment:
    """BundleAdjustment(camera, level, numParameters) — optimizePose (src/bundle_adjustment.cpp:30-166), twoViewBA
    (:397-478) and localBA (:480-625).

    ref_visibility is the member m_refVisibility: optimizePose's residual step reads the flags the
    previous call left (a fresh object returns NaN and moves nothing), see include/svo_c.h."""

    def __init__(self, camera, level=0, num_parameters=6, ctx=None):
        self.camera, self.level = camera, int(level)
        self.ctx = ctx or default_context()
        self.ref_visibility = np.zeros(0, np.uint8)
        self.last_status = None

    def optimize_pose(self, frame):
        n = len(frame.features)
        if n == 0:  # :37-38
            return 0.0
        vis = np.zeros(n, np.uint8)
        k = min(n, len(self.ref_visibility))
        vis[:k] = self.ref_visibility[:k]  # m_refVisibility.resize(n, false)
        bearing = np.array([f.bearing_vec for f in frame.features], np.float64).reshape(n, 3)
        has = np.array([f.point is not None for f in frame.features], np.uint8)
        point = np.array([f.point.position if f.point is not None else (0.0, 0.0, 0.0) for f in frame.features],
                         np.float64).reshape(n, 3)
        poses = np.ascontiguousarray(frame.abs_pose, np.float64).reshape(1, 7).copy()
        err, st = pose_optimize_batch([0, n], bearing, point, has, vis, poses, self.ctx)
        self.ref_visibility = vis
        frame.abs_pose = poses[0].copy()
        self.last_status = int(st[0])
        return float(err[0])

    def _adjust(self, map_, frames, fixed, points, edges, reprojection_error, structure_iterations):
        """The shared tail of two_view_ba / local_ba: one problem of `frames` (fixed flags), `points` and `edges`
        (frame index, point index, feature; grouped by point), 10 iterations with Huber width reprojection_error;
        poses of the free frames and all positions written back, then Map.remove_feature for every edge whose
        e2 exceeds reprojection_error^2, in edge order.  Returns (init chi, final chi, edges over the threshold)."""
        n_free = len(frames) - int(np.count_nonzero(fixed))
        if n_free > BA_MAX_FRAMES:  # (fixed frames are not limited)
            raise ValueError(f"bundle adjustment over {n_free} frames free to move (at most {BA_MAX_FRAMES})")
        poses = np.array([np.asarray(f.abs_pose, np.float64).reshape(7) for f in frames], np.float64).reshape(-1, 7)
        rows = np.fromiter((p._i for p in points), np.int64, count=len(points))
        pos = np.ascontiguousarray(_PT.pos[rows], np.float64).reshape(-1, 3)
        of = np.fromiter((e[0] for e in edges), np.int32, count=len(edges))
        op = np.fromiter((e[1] for e in edges), np.int32, count=len(edges))
        px = _rows([e[2].pixel_position for e in edges], 2) if edges else np.zeros((0, 2))
        r = bundle_adjust_batch(self.camera, [0, len(frames)], [0, len(points)], [0, len(edges)], poses, fixed, pos,
                                of, op, px, reprojection_error, 10, structure_iterations, False, self.ctx)
        self.last_status = int(r.status[0])
        for i, fr in enumerate(frames):
            if not fixed[i]:
                fr.abs_pose = poses[i].copy()
        if len(points):  # every position in one assignment, one bump of the points' version
            _PT.pos[rows] = pos
            Point._ver += 1
        over = np.nonzero(r.obs_chi2 > reprojection_error * reprojection_error)[0]
        for k in over:  # (:461-476, :598-609)
            map_.remove_feature(edges[k][2])
        return float(r.init_chi[0]), float(r.final_chi[0]), len(over)

    def two_view_ba(self, fst_frame, sec_frame, map, reprojection_error):
        """twoViewBA (src/bundle_adjustment.cpp:397-478): fst_frame fixed, sec_frame free, one point vertex per
        feature of fst_frame that has a point, its edge in fst_frame and the edge of Point::findFeature(sec_frame),
        Huber width reprojection_error, 10 iterations; both poses and all positions written back, then
        map.remove_feature for every edge with e2 > reprojection_error^2 in edge order."""
        in_sec = {}
        for f in sec_frame.features:  # Point::findFeature: the first feature of the frame that holds the point
            if f.point is not None:
                in_sec.setdefault(id(f.point), f)
        points, edges = [], []
        for f in fst_frame.features:
            if f.point is None:
                continue
            g = in_sec.get(id(f.point))
            if g is None:
                raise ValueError("a point of the first frame is not observed in the second frame")
            edges += [(0, len(points), f), (1, len(points), g)]
            points.append(f.point)
        return self._adjust(map, [fst_frame, sec_frame], np.array([1, 0], np.uint8), points, edges,
                            reprojection_error, 0)

    def local_ba(self, map, reprojection_error):
        """localBA (src/bundle_adjustment.cpp:480-625): every frame of map.key_frames free; the points are those
        with more than one observation that a keyframe observes; an observing frame outside the keyframe list
        becomes a fixed frame; StructureOnlySolver first (10 iterations), then 10 joint iterations; write back;
        map.remove_feature for every edge over the threshold.  The reference walks a std::set of shared_ptr, that
        is, the points in pointer order; here they are taken in first-seen order (keyframe order, then feature
        order), so the result does not depend on the allocator.  More than 16 keyframes raise."""
        frames = list(map.key_frames)
        index = {id(fr): i for i, fr in enumerate(frames)}
        n_key = len(frames)
        points, seen = [], set()
        for fr in map.key_frames:
            for f in fr.features:
                p = f.point
                if p is not None and p.number_observation() > 1 and id(p) not in seen:
                    seen.add(id(p))
                    points.append(p)
        edges = []
        for j, p in enumerate(points):
            for f in p.features:
                i = index.get(id(f.frame))
                if i is None:  # a neighbour keyframe: fixed (:532-540)
                    i = index[id(f.frame)] = len(frames)
                    frames.append(f.frame)
                edges.append((i, j, f))
        fixed = np.zeros(len(frames), np.uint8)
        fixed[n_key:] = 1
        return self._adjust(map, frames, fixed, points, edges, reprojection_error, 10)


# ---------------------------------------------------------------- two-view map initialisation
def _c_f64(a, shape, name):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shape):
        raise ValueError(f"{name} must be a C-contiguous float64 array of shape {shape} (it is updated in place)")
    return a


def triangulate_batch(camera, feat_off, ref_poses, cur_poses, ref_px, cur_px, ctx=None):
    """svo_triangulate_dlt (algorithm::triangulate3DWorldPoints, src/algorithm.cpp:553-566) over arrays: pair p
    owns matches feat_off[p]:feat_off[p+1], posed ref_poses[p] / cur_poses[p].  Returns points_world (n, 3)."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    P = len(feat_off) - 1
    n = int(feat_off[-1])
    ref_poses = np.ascontiguousarray(ref_poses, np.float64).reshape(P, 7)
    cur_poses = np.ascontiguousarray(cur_poses, np.float64).reshape(P, 7)
    ref_px = np.ascontiguousarray(ref_px, np.float64).reshape(n, 2)
    cur_px = np.ascontiguousarray(cur_px, np.float64).reshape(n, 2)
    out = np.zeros((n, 3))
    cam = camera.as_c()
    check(lib().svo_triangulate_dlt(ctx.handle, ctypes.byref(cam), P, ptr(feat_off), ptr(ref_poses), ptr(cur_poses),
                                    ptr(ref_px), ptr(cur_px), ptr(out)))
    return out


class TwoViewResult:
    """Outputs of two_view_init_batch (include/svo_c.h svo_two_view_init): F (P, 3, 3), counts (P, 4), winner (P,),
    cur_poses (P, 7; NaN rows for failed pairs), median_depth (P,), n_valid (P,), points_world (n, 3), valid (n,),
    survivor (n,), depth (n,)."""
    __slots__ = ("F", "counts", "winner", "cur_poses", "median_depth", "n_valid", "points_world", "valid", "survivor",
                 "depth")


def two_view_init_batch(camera, feat_off, E, ref_poses, ref_px, cur_px, map_scale, cell_size, ctx=None):
    """svo_two_view_init over arrays (System::processSecondFrame from the essential matrix on,
    src/system.cpp:144-223).  ref_px / cur_px ((n, 2) float64, C-contiguous) are Sampson-corrected in place."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    P = len(feat_off) - 1
    n = int(feat_off[-1])
    E = np.ascontiguousarray(E, np.float64).reshape(P, 9)
    ref_poses = np.ascontiguousarray(ref_poses, np.float64).reshape(P, 7)
    _c_f64(ref_px, (n, 2), "ref_px")
    _c_f64(cur_px, (n, 2), "cur_px")
    r = TwoViewResult()
    r.F = np.zeros((P, 3, 3))
    r.counts = np.zeros((P, 4), np.int32)
    r.winner = np.zeros(P, np.int32)
    r.cur_poses = np.full((P, 7), np.nan)  # the call leaves a failed pair's row alone
    r.median_depth = np.zeros(P)
    r.n_valid = np.zeros(P, np.int32)
    r.points_world = np.zeros((n, 3))
    r.valid = np.zeros(n, np.uint8)
    r.survivor = np.zeros(n, np.int32)
    r.depth = np.zeros(n)
    cam = camera.as_c()
    check(lib().svo_two_view_init(ctx.handle, ctypes.byref(cam), P, ptr(feat_off), ptr(E), ptr(ref_poses),
                                  float(map_scale), int(cell_size), ptr(ref_px), ptr(cur_px), ptr(r.F), ptr(r.counts),
                                  ptr(r.winner), ptr(r.cur_poses), ptr(r.median_depth), ptr(r.n_valid),
                                  ptr(r.points_world), ptr(r.valid), ptr(r.survivor), ptr(r.depth)))
    return r


def _set_pixels(frame, px):
    """Feature.pixel_position of every feature of `frame` <- the rows of px, with one bump of the frame's feature
    version (the rows of one frozen copy, as Feature._many lays them out)."""
    rows = _frozen(px)
    for f, row in zip(frame.features, rows):
        f._px = row
    frame._feat_ver[0] += 1


def two_view_initialize(ref_frame, cur_frame, E, map_scale, cell_size, ctx=None):
    """What System::processSecondFrame does to the two frames between computeEssentialMatrix and twoViewBA
    (src/system.cpp:144-223): Sampson-corrected pixel positions in both frames, cur_frame.abs_pose, one Point per
    valid match linked both ways, and the features without a point erased from both frames (order kept).
    Feature i of ref_frame matches feature i of cur_frame.  Returns (ok, median depth before scaling, number of
    points); ok False when recoverPose fails: the pixels stay corrected, nothing else changes (:152-156)."""
    n = ref_frame.number_observation()
    if cur_frame.number_observation() != n:
        raise ValueError("ref_frame and cur_frame must hold the same number of (matched) features")
    # (the gathers also form every bearing from the uncorrected pixel, as the reference's Feature constructor did)
    ref_px = np.array(ref_frame.feature_arrays()[0], np.float64).reshape(n, 2)
    cur_px = np.array(cur_frame.feature_arrays()[0], np.float64).reshape(n, 2)
    r = two_view_init_batch(ref_frame.camera, [0, n], np.asarray(E, np.float64).reshape(1, 9),
                            np.asarray(ref_frame.abs_pose, np.float64).reshape(1, 7), ref_px, cur_px, map_scale,
                            cell_size, ctx)
    _set_pixels(ref_frame, ref_px)  # sampsonCorrection (src/algorithm.cpp:233-234)
    _set_pixels(cur_frame, cur_px)
    if r.winner[0] < 0:
        return False, float("nan"), 0
    cur_frame.abs_pose = r.cur_poses[0].copy()
    for i in r.survivor[:int(r.n_valid[0])]:  # (:201-209)
        point = Point(r.points_world[i])
        fr, fc = ref_frame.features[i], cur_frame.features[i]
        fr.set_point(point)
        fc.set_point(point)
        point.add_feature(fr)
        point.add_feature(fc)
    for fr in (ref_frame, cur_frame):  # remove_if(m_point == nullptr) (:217-223)
        fr.features = [f for f in fr.features if f.point is not None]
    return True, float(r.median_depth[0]), int(r.n_valid[0])


# ---------------------------------------------------------------- sparse optical flow (pyramidal Lucas-Kanade)
def klt_track_batch(ref_set, cur_set, frames, feat_off, ref_px, cur_px, win=11, max_level=3, max_iterations=30,
                    epsilon=1e-4, min_eig_threshold=1e-4, trace=False, ctx=None):
    """svo_klt_track over arrays: pair p tracks points feat_off[p]:feat_off[p+1] from frame frames[p][0] of ref_set
    into frame frames[p][1] of cur_set, starting at cur_px (the initial flow; not modified).  Returns (cur (n, 2),
    status (n,) uint8, median_disparity (P,)), and the per-level trace (n, max_level + 1, 2) int32 last with
    trace=True (include/svo_c.h lists the exit codes)."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    P = len(feat_off) - 1
    n = int(feat_off[-1]) if P >= 0 else 0
    frames = np.ascontiguousarray(frames, np.int32).reshape(P, 2)
    ref_px = np.ascontiguousarray(ref_px, np.float64).reshape(n, 2)
    cur = np.array(cur_px, np.float64).reshape(n, 2)
    status = np.zeros(n, np.uint8)
    median = np.zeros(P)
    tr = np.zeros((n, max(int(max_level), 0) + 1, 2), np.int32) if trace else None
    check(lib().svo_klt_track(ctx.handle, ref_set.handle, cur_set.handle, P, ptr(frames), ptr(feat_off), ptr(ref_px),
                              ptr(cur), int(win), int(max_level), int(max_iterations), float(epsilon),
                              float(min_eig_threshold), ptr(status), ptr(tr), ptr(median)))
    return (cur, status, median, tr) if trace else (cur, status, median)


def compute_optical_flow_sparse(ref_frame, cur_frame, patch_size, disparity_threshold, ctx=None):
    """algorithm::computeOpticalFlowSparse(refFrame, curFrame, patchSize, disparityThreshold)
    (src/algorithm.cpp:29-107): the ref frame's features tracked into the cur frame (window patch_size, 4 levels, 30
    iterations, eps 1e-4, initial flow = the ref positions); a Feature(cur, px, 0.0, 0.0, 0) is added to cur_frame
    per tracked point, in order; False when the median disparity is below the threshold (the cur features stay, the
    ref frame is untouched: the reference's own order); otherwise the untracked features leave ref_frame (order
    kept) and the result is True.  No tracked point gives a NaN median and hence True, as in the reference."""
    n = ref_frame.number_observation()
    ref_px = np.array(ref_frame.feature_arrays()[0], np.float64).reshape(n, 2)
    cur, status, median = klt_track_batch(ref_frame.image_pyramid.set, cur_frame.image_pyramid.set, [[0, 0]], [0, n],
                                          ref_px, ref_px, int(patch_size), 3, 30, 1e-4, ctx=ctx)[:3]
    tracked = status == 1
    new = Feature._many(cur_frame, cur[tracked], level=0, gradient_magnitude=[0.0] * int(tracked.sum()))
    cur_frame.features.extend(new)
    if median[0] < disparity_threshold:
        return False
    ref_frame.features = [f for f, t in zip(ref_frame.features, tracked) if t]
    return True


# ---------------------------------------------------------------- essential-matrix RANSAC
class EssentialResult:
    """E (P, 3, 3), mask (n,) uint8, n_inliers / iterations / status (P,), best (P, 2); with trace=True also hyp_E
    (P, max_iterations, 10, 3, 3) and hyp_count (P, max_iterations, 10)."""


def essential_score_batch(camera, feat_off, hyp_off, E_hyp, ref_px, cur_px, threshold=1.0, want_mask=True, ctx=None):
    """svo_essential_score over arrays: the inlier count of every model of E_hyp (pair p owns models
    hyp_off[p]:hyp_off[p+1]) among its pair's matches, and per pair the mask of its first model with the strictly
    largest count.  Returns (counts (m,) int32, mask (n,) uint8 or None)."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    hyp_off = np.ascontiguousarray(hyp_off, np.int32)
    P = len(feat_off) - 1
    if len(hyp_off) != P + 1:
        raise ValueError("hyp_off and feat_off differ in length")
    n, m = int(feat_off[-1]), int(hyp_off[-1])
    E_hyp = np.ascontiguousarray(E_hyp, np.float64).reshape(m, 9)
    ref_px = np.ascontiguousarray(ref_px, np.float64).reshape(n, 2)
    cur_px = np.ascontiguousarray(cur_px, np.float64).reshape(n, 2)
    counts = np.zeros(m, np.int32)
    mask = np.zeros(n, np.uint8) if want_mask else None
    cam = camera.as_c()
    check(lib().svo_essential_score(ctx.handle, ctypes.byref(cam), P, ptr(feat_off), ptr(hyp_off), ptr(E_hyp),
                                    ptr(ref_px), ptr(cur_px), float(threshold), ptr(counts), ptr(mask)))
    return counts, mask


def essential_ransac_batch(camera, feat_off, ref_px, cur_px, threshold=1.0, confidence=0.999, max_iterations=1000,
                           seed=0, trace=False, ctx=None):
    """svo_essential_ransac over arrays (the cv::findEssentialMat of algorithm::computeEssentialMatrix,
    src/algorithm.cpp:130, for a batch of pairs; include/svo_c.h states the contract).  Pair p owns matches
    feat_off[p]:feat_off[p+1] of ref_px / cur_px ((n, 2), not modified)."""
    ctx = ctx or default_context()
    feat_off = np.ascontiguousarray(feat_off, np.int32)
    P = len(feat_off) - 1
    n = int(feat_off[-1]) if P >= 0 else 0
    ref_px = np.ascontiguousarray(ref_px, np.float64).reshape(n, 2)
    cur_px = np.ascontiguousarray(cur_px, np.float64).reshape(n, 2)
    r = EssentialResult()
    r.E = np.zeros((P, 3, 3))
    r.mask = np.zeros(n, np.uint8)
    r.n_inliers = np.zeros(P, np.int32)
    r.iterations = np.zeros(P, np.int32)
    r.best = np.zeros((P, 2), np.int32)
    r.status = np.zeros(P, np.int32)
    mi = max(int(max_iterations), 0)
    r.hyp_E = np.zeros((P, mi, 10, 3, 3)) if trace else None
    r.hyp_count = np.zeros((P, mi, 10), np.int32) if trace else None
    cam = camera.as_c()
    check(lib().svo_essential_ransac(ctx.handle, ctypes.byref(cam), P, ptr(feat_off), ptr(ref_px), ptr(cur_px),
                                     float(threshold), float(confidence), int(max_iterations),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(r.E), ptr(r.mask), ptr(r.n_inliers),
                                     ptr(r.iterations), ptr(r.best), ptr(r.status), ptr(r.hyp_E), ptr(r.hyp_count)))
    return r


def compute_essential_matrix(ref_frame, cur_frame, repro_error, threshold_corresponding_points, seed=0, ctx=None):
    """algorithm::computeEssentialMatrix(refFrame, curFrame, reproError, thresholdCorrespondingPoints, E)
    (src/algorithm.cpp:109-171): feature i of ref_frame matches feature i of cur_frame; the RANSAC (confidence 0.999,
    threshold repro_error px, at most 1000 samples) runs on the device, the matches it rejects are erased from both
    frames (order kept), and the result is (ok, E): ok when both frames keep more than the threshold.  A pair without
    a model keeps no feature and returns a zero E."""
    n = ref_frame.number_observation()
    if cur_frame.number_observation() != n:
        raise ValueError("the frames differ in their number of features")
    ref_px = np.array(ref_frame.feature_arrays()[0], np.float64).reshape(n, 2)
    cur_px = np.array(cur_frame.feature_arrays()[0], np.float64).reshape(n, 2)
    r = essential_ransac_batch(ref_frame.camera, [0, n], ref_px, cur_px, float(repro_error), 0.999, 1000, seed, ctx=ctx)
    keep = r.mask == 1
    for fr in (ref_frame, cur_frame):  # one assignment per frame: one bump of its cached feature arrays
        fr.features = [f for f, k in zip(fr.features, keep) if k]
    ok = (ref_frame.number_observation() > threshold_corresponding_points and
          cur_frame.number_observation() > threshold_corresponding_points)
    return ok, r.E[0].copy()


# ---------------------------------------------------------------- the tracker: algorithm:: scalars and System
def compute_relative_pose(ref_frame, cur_frame):
    """algorithm::computeRelativePose (src/algorithm.cpp:705-709): T_cur_ref = cur.absPose * ref.absPose^-1."""
    return pose_compose(cur_frame.abs_pose, pose_inverse(ref_frame.abs_pose))


def normalized_depth_camera(frame):
    """algorithm::normalizedDepthCamera(frame, out) (src/algorithm.cpp:601-608): |world2camera(point)| of every
    feature (each must have a point)."""
    if not len(frame.features):
        return np.zeros(0)
    rows = _point_rows(frame.features)
    if (rows < 0).any():
        raise ValueError("normalized_depth_camera: a feature without a point (the reference dereferences it)")
    pc = _quat_rotate(frame.abs_pose[:4], _PT.pos[rows]) + frame.abs_pose[4:]
    return np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])


def _nth_element(a, nth):
    """libstdc++'s std::nth_element(a, a + nth, a + len(a)) on a list of floats, in place: introselect (median of
    three to the front, unguarded Hoare partition, heap select after 2 log2 n rounds, insertion sort of the last
    <= 3), so that a[nth - 1] is what the reference reads for an even length (tests/test_system.py checks it against
    the toolchain's own function)."""
    first, last = 0, len(a)
    if first == last or nth == last:
        return
    depth = 2 * (last.bit_length() - 1)
    while last - first > 3:
        if depth == 0:  # __heap_select(first, nth + 1, last); iter_swap(first, nth)
            middle = nth + 1

            def adjust(hole, n, value):  # __adjust_heap + __push_heap on a[first:first + n]
                top, child = hole, hole
                while child < (n - 1) // 2:
                    child = 2 * (child + 1)
                    if a[first + child] < a[first + child - 1]:
                        child -= 1
                    a[first + hole] = a[first + child]
                    hole = child
                if n % 2 == 0 and child == (n - 2) // 2:
                    child = 2 * (child + 1)
                    a[first + hole] = a[first + child - 1]
                    hole = child - 1
                parent = (hole - 1) // 2
                while hole > top and a[first + parent] < value:
                    a[first + hole] = a[first + parent]
                    hole = parent
                    parent = (hole - 1) // 2
                a[first + hole] = value

            n = middle - first
            if n >= 2:  # __make_heap
                parent = (n - 2) // 2
                while True:
                    adjust(parent, n, a[first + parent])
                    if parent == 0:
                        break
                    parent -= 1
            for i in range(middle, last):
                if a[i] < a[first]:  # __pop_heap(first, middle, i)
                    value = a[i]
                    a[i] = a[first]
                    adjust(0, n, value)
            a[first], a[nth] = a[nth], a[first]
            return
        depth -= 1
        mid = first + (last - first) // 2
        x, y, z = first + 1, mid, last - 1  # __move_median_to_first(first, first + 1, mid, last - 1)
        if a[x] < a[y]:
            m = y if a[y] < a[z] else (z if a[x] < a[z] else x)
        else:
            m = x if a[x] < a[z] else (z if a[y] < a[z] else y)
        a[first], a[m] = a[m], a[first]
        pivot = a[first]
        lo, hi = first + 1, last  # __unguarded_partition(first + 1, last, first)
        while True:
            while a[lo] < pivot:
                lo += 1
            hi -= 1
            while pivot < a[hi]:
                hi -= 1
            if not lo < hi:
                break
            a[lo], a[hi] = a[hi], a[lo]
            lo += 1
        if lo <= nth:
            first = lo
        else:
            last = lo
    for i in range(first + 1, last):  # __insertion_sort
        v = a[i]
        j = i
        while j > first and v < a[j - 1]:
            a[j] = a[j - 1]
            j -= 1
        a[j] = v


def compute_median(values):
    """algorithm::computeMedian(input) (src/algorithm.cpp:813-832): std::nth_element at size / 2; an even length
    averages vec[mid - 1], as nth_element left it, with vec[mid]; NaN for an empty input."""
    vec = np.asarray(values, np.float64).reshape(-1).tolist()
    if not vec:
        return float("nan")
    mid = len(vec) // 2
    _nth_element(vec, mid)
    return vec[mid] if len(vec) % 2 else (vec[mid - 1] + vec[mid]) / 2.0


def compute_number_projected_points(cur_frame):
    """algorithm::computeNumberProjectedPoints (src/algorithm.cpp:783-804): the features with a point whose bearing,
    stretched to the point's distance from the camera centre and moved by T_cur_lastKeyframe, projects inside the
    5-px border."""
    rel = compute_relative_pose(cur_frame.last_keyframe, cur_frame)
    C = cur_frame.camera_in_world()
    cam = cur_frame.camera
    n = 0
    for f in cur_frame.features:
        if f.point is None:
            continue
        cur_point = _quat_rotate(rel[:4], f.bearing_vec * _norm3(f.point.position - C)) + rel[4:]
        if cam.is_in_frame(cam.project2d(cur_point), 5.0):
            n += 1
    return n


class Config:
    """The fields of the reference's Config (include/config.hpp) that src/system.cpp reads, with the defaults of its
    config/config.json and resource/kitti.yaml, plus what this project adds: ransac_seed (the RANSAC sampler),
    map_cell_seed (the map's cell order), max_keyframes (the literal 7 of src/system.cpp:436) and median_mode
    (ImageAlignment's robust scale), and d0..d4, the lens coefficients (k1, k2, p1, p2, k3) of the reference's
    PinholeCamera, all 0 by default (KITTI's rectified images), and pixel_format / gray16_shift, what add_image is handed
    ("gray8" by default; include/svo_c.h, "pixel formats").  Visualisation and logging are not part of it."""

    def __init__(self, **kw):
        self.img_width, self.img_height = 1241, 376
        self.fx = self.fy = 721.5377
        self.cx, self.cy = 609.5593, 172.8540
        self.d0 = self.d1 = self.d2 = self.d3 = self.d4 = 0.0
        self.pixel_format = "gray8"  # what add_image is handed: gray8, bgr8, rgb8, bgra8, rgba8 or gray16
        self.gray16_shift = 8        # gray16: Y = min(255, v >> shift)
        self.patch_size_optical_flow = 11
        self.patch_size_image_alignment = 5
        self.min_level_image_pyramid = 0
        self.max_level_image_pyramid = 3
        self.cell_pixel_size = 30
        self.threshold_gradient_magnitude = 50
        self.desired_detected_points_for_initialization = 200
        self.min_detected_points_success_initialization = 100
        self.disparity_threshold = 5.0
        self.init_map_scale_factor = 1.0
        self.ransac_seed = 0
        self.map_cell_seed = 0
        self.max_keyframes = 7
        self.median_mode = MEDIAN_REFERENCE
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(f"Config has no field {k!r}")
            setattr(self, k, v)


class System:
    """System(config) (include/system.hpp, src/system.cpp:15-511): the state machine that turns images into poses,
    addImage -> processFirstFrame / processSecondFrame / processNewFrame / relocalisation, each step one of the
    device-backed classes above in the reference's order.

    add_image takes RAW images in Config.pixel_format (colour and 16-bit frames become grey on the device first); with
    any of Config.d0..d4 non-zero each is undistorted on the device ahead of its pyramid (the reference's System never
    calls PinholeCamera::undistortImage), and everything downstream is the plain pinhole model on undistorted pixels.

    Deliberate differences from the reference:
      * the depth estimator runs without its worker thread, i.e. the reference's own m_thread == nullptr branch
        (addFrame = updateFilters, addKeyframe = initializeFilters), so a run is a function of its images and seeds;
      * the seed-age rule (src/depth_estimator.cpp:220) compares a static counter the reference never advances: it
        is inert there and absent here;
      * the map's cell order and the RANSAC samples are seeded (Config.map_cell_seed, Config.ransac_seed) where
        the reference draws from std::random_device / cv::RNG;
      * DepthEstimator.remove_keyframe takes effect at the next add_frame / add_keyframe (there: at the worker's
        next update).
    Visualisation and logging are left out; report_summary returns the counts."""

    # System::Status / System::Result (include/system.hpp:23-38; "Procese" is the reference's spelling)
    PROCESS_FIRST_FRAME, PROCESS_SECOND_FRAME, PROCESS_NEW_FRAME, PROCESS_RELOCALIZATION = 0, 1, 2, 3
    SUCCESS, FAILED, KEYFRAME = 0, 1, 2

    def __init__(self, config=None, ctx=None, instrument=False):  # :15-32
        c = self.config = config or Config()
        self.instrument = bool(instrument)  # fill timings and ba_removed (tests, tools/system_time.py); off: no cost
        self.ctx = ctx or default_context()
        self.camera = PinholeCamera(c.img_width, c.img_height, c.fx, c.fy, c.cx, c.cy, c.d0, c.d1, c.d2, c.d3, c.d4)
        self.alignment = ImageAlignment(c.patch_size_image_alignment, c.min_level_image_pyramid,
                                        c.max_level_image_pyramid, 6, self.ctx, c.median_mode)
        self.feature_selector = FeatureSelection(c.img_width, c.img_height, c.cell_pixel_size, self.ctx)
        self.map = Map(self.camera, c.cell_pixel_size, c.map_cell_seed, self.ctx)
        self.depth_estimator = DepthEstimator(self.ctx, self.map)
        self.bundler = BundleAdjustment(self.camera, 0, 6, self.ctx)
        self.active_keyframe = None
        self.ref_frame = None
        self.cur_frame = None
        self.prediction_relative_pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
        self.status = System.PROCESS_FIRST_FRAME
        self.last_result = System.FAILED
        self.ba_removed = []   # instrument: (frame id, feature index before the BA) of what the last BA removed
        self.timings = {}      # instrument: host seconds per step of the last add_image

    def set_status(self, status):
        """The relocalisation branch is never entered by the reference itself (nothing sets the status): tests and
        callers reach it through this setter."""
        self.status = int(status)

    def _timed(self, name, fn, *a):
        if not self.instrument:
            return fn(*a)
        t0 = time.perf_counter()
        r = fn(*a)
        self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0
        return r

    def add_image(self, img, timestamp=0):  # :34-76
        if self.instrument:
            self.timings, self.ba_removed = {}, []
        c = self.config
        self.cur_frame = self._timed("frame", Frame, self.camera, img, c.max_level_image_pyramid + 1, timestamp,
                                     self.active_keyframe, self.ctx, c.pixel_format, c.gray16_shift)
        res = System.FAILED
        if self.status == System.PROCESS_NEW_FRAME:
            res = self.process_new_frame()
        elif self.status == System.PROCESS_SECOND_FRAME:
            res = self.process_second_frame()
        elif self.status == System.PROCESS_FIRST_FRAME:
            res = self.process_first_frame()
        elif self.status == System.PROCESS_RELOCALIZATION:
            res = self.relocalize_frame(self.map.get_closest_keyframe(self.cur_frame))
        if self.ref_frame is not None:
            self.prediction_relative_pose = compute_relative_pose(self.ref_frame, self.cur_frame)
        self.last_result = res
        if res == System.FAILED:
            return False
        self.ref_frame = self.cur_frame
        return True

    def _select(self, frame):
        c = self.config
        self._timed("select", self.feature_selector.gradient_magnitude_with_ssc, frame, c.threshold_gradient_magnitude,
                    c.desired_detected_points_for_initialization, True)

    def process_first_frame(self):  # :78-115
        c, cur = self.config, self.cur_frame
        self._select(cur)
        if cur.number_observation() < c.min_detected_points_success_initialization:
            return System.FAILED
        cur.set_keyframe()
        self.active_keyframe = cur
        self.map.add_keyframe(cur)
        self.status = System.PROCESS_SECOND_FRAME
        return System.SUCCESS

    def _run_ba(self, frames, fn, *a):
        """fn(*a) (a windowed BA) with ba_removed <- the features it removed from `frames`."""
        if not self.instrument:
            return fn(*a)
        before = [(fr, list(fr.features)) for fr in frames]
        r = self._timed("ba", fn, *a)
        for fr, feats in before:
            left = {id(f) for f in fr.features}
            self.ba_removed += [(fr.id, i) for i, f in enumerate(feats) if id(f) not in left]
        return r

    def process_second_frame(self):  # :117-302
        c, ref, cur = self.config, self.ref_frame, self.cur_frame
        if not self._timed("klt", compute_optical_flow_sparse, ref, cur, c.patch_size_optical_flow,
                           c.disparity_threshold, self.ctx):
            return System.FAILED
        threshold = int(c.min_detected_points_success_initialization * 0.5)
        ok, E = self._timed("essential", compute_essential_matrix, ref, cur, 1.0, threshold, c.ransac_seed, self.ctx)
        if not ok:
            return System.FAILED
        ok, _, _ = self._timed("two_view", two_view_initialize, ref, cur, E, c.init_map_scale_factor,
                               c.cell_pixel_size, self.ctx)
        if not ok:
            return System.FAILED
        self._run_ba([ref, cur], self.bundler.two_view_ba, ref, cur, self.map, 2.0)
        cur.set_keyframe()
        self.active_keyframe = cur
        depths = normalized_depth_camera(cur)
        median_depth = compute_median(depths)
        min_depth = float(depths.min())
        self.feature_selector.set_existing_features(cur.features)
        self._select(cur)
        self.depth_estimator.add_keyframe(cur, median_depth, 0.5 * min_depth)
        self.map.add_keyframe(cur)
        self.status = System.PROCESS_NEW_FRAME
        return System.SUCCESS

    def process_new_frame(self):  # :304-446
        ref, cur = self.ref_frame, self.cur_frame
        cur.abs_pose = pose_compose(self.prediction_relative_pose, ref.abs_pose)
        self._timed("align", self.alignment.align, ref, cur)
        self._timed("reproject", self.map.reproject_map, ref, cur, [])
        self._timed("candidates", self.map.add_candidate_to_frame, cur)
        if not self.compute_tracking_quality(cur, ref.number_observation_with_points()):
            cur.abs_pose = np.array(ref.abs_pose, np.float64)
            return System.SUCCESS
        depths = normalized_depth_camera(cur)
        depth_mean = compute_median(depths)
        depth_min = float(depths.min())
        if self.need_keyframe(depths, depth_mean):
            self._timed("depth", self.depth_estimator.add_frame, cur)
            return System.SUCCESS
        cur.set_keyframe()
        self.map.add_keyframe(cur)
        self.active_keyframe = cur
        self._run_ba(list(self.map.key_frames), self.bundler.local_ba, self.map, 2.0)
        self.feature_selector.set_existing_features(cur.features)
        self._select(cur)
        self.depth_estimator.add_keyframe(cur, depth_mean, depth_min * 0.5)
        if self.map.size_keyframes() > self.config.max_keyframes:  # :436-442
            furthest = self.map.get_furthest_keyframe(cur.camera_in_world())
            self.depth_estimator.remove_keyframe(furthest)
            self.map.remove_frame(furthest)
        return System.KEYFRAME

    def relocalize_frame(self, closest_keyframe):
        """relocalizeFrame (:448-457).  A closest keyframe without a last keyframe (the very first one) raises in
        ImageAlignment.align, where the reference dereferences the null pointer."""
        if closest_keyframe is None:
            return System.FAILED
        self._timed("align", self.alignment.align, closest_keyframe, self.cur_frame)
        return System.SUCCESS

    @staticmethod
    def compute_tracking_quality(frame, ref_frame_number_observations):  # :459-472
        cur = frame.number_observation()
        if cur < 50:
            return False
        return not (int(ref_frame_number_observations) - cur > 40)

    def need_keyframe(self, depths_in_cur_frame, scene_depth_mean):
        """needKeyframe (:474-511).  As in the reference, True means that NO keyframe is needed: diffId < 3 (the
        other quantities it computes only feed its log)."""
        cur = self.cur_frame
        return cur.id - cur.last_keyframe.id < 3

    def write_in_file(self, f):  # :635-640
        from . import trajectory
        trajectory.write_in_file(self.ref_frame, f)

    def report_summary(self):
        """reportSummary (:513-552) as a dict instead of log lines.  The reference walks m_allFrames, which it never
        fills; here the frames are the keyframes of the map and the reference / current frame."""
        frames = list(self.map.key_frames)
        for fr in (self.ref_frame, self.cur_frame):
            if fr is not None and all(fr is not k for k in frames):
                frames.append(fr)
        points, n_features = set(), 0
        rows = []
        for fr in frames:
            n_features += fr.number_observation()
            points.update(id(f.point) for f in fr.features if f.point is not None)
            rows.append(dict(id=fr.id, keyframe=fr.is_keyframe(), features=fr.number_observation(),
                             features_with_points=fr.number_observation_with_points(),
                             last_keyframe=-1 if fr.last_keyframe is None else fr.last_keyframe.id))
        return dict(frames=rows, features=n_features, points=len(points),
                    filters=self.depth_estimator.number_filters(), candidates=len(self.map.candidates),
                    keyframes=self.map.size_keyframes())
