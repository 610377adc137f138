"""Pixel formats (include/svo_c.h, "pixel formats"): what needs no GPU.

  * the numpy restatement (tests/convert_ref.py) over all 2^24 colours: grey stays grey, the range is 0..255, and it lies
    within 0.51 of 0.299 R + 0.587 G + 0.114 B (the largest deviation is 0.506: the weights themselves are rounded);
  * the anchor on committed bytes: the restatement of the RGB crop of the reference's image_1.png equals the same window
    of refimages.npz["image_1"] (tests/golden/make_golden_convert.py, make_golden_refimages.py);
  * svo_image_layout_bytes: sizes and every error case, as a code with a text;
  * tests/cpp/convert_model.cpp: the kernel's per-thread body (csrc/convert_math.h) over every thread of the launch for
    every shape of the GPU edge list, against a scalar loop, with every load inside the layout's bytes;
  * the mirrors' validation, and that calls without a pixel format reach the entry points they reached before;
  * the scene of the System test: the restatement tracker still initialises on the colour frames' grey images.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import convert_ref as CR
import svo_amd
import system_ref as SR
import system_scene as SC
import test_system as TS
from svo_amd import _capi, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def colour_scene():
    """The eight frames of tests/system_scene.py as RGB, (R, G, B) = (g, g, 255 - g): the mapping the issue names first.
    Its grey image is 0.772 g + 29.6, so the texture keeps three quarters of its contrast, and a BGR / RGB mix-up gives
    0.412 g + 88.5 instead.  (B = g >> 1, the fallback, was not needed: see test_scene_still_initialises_in_colour.)"""
    imgs, gt = TS.sequence()
    rgb = np.stack([imgs, imgs, 255 - imgs], axis=-1)
    rgb.flags.writeable = False
    return rgb, gt


# ---------------------------------------------------------------- the restatement
def test_restatement_over_all_colours():
    g, b = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    worst = 0.0
    for r in range(256):
        y = CR.luma(np.full_like(g, r), g, b)
        assert y.dtype == np.uint8  # (so the range is 0..255; the next line shows nothing was cut off on the way)
        full = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
        assert int(full.max()) <= 255 and np.array_equal(full, y)
        worst = max(worst, float(np.abs(y - (0.299 * r + 0.587 * g + 0.114 * b)).max()))
    print("largest |Y - (0.299 R + 0.587 G + 0.114 B)| = %.4f" % worst)
    assert worst <= 0.51
    v = np.arange(256)
    assert np.array_equal(CR.luma(v, v, v), v)
    assert 4899 + 9617 + 1868 == 1 << 14


def test_restatement_formats():
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    want = CR.luma(px[..., 0], px[..., 1], px[..., 2])
    assert np.array_equal(CR.convert_ref(px[..., :3], "rgb8"), want)
    assert np.array_equal(CR.convert_ref(px, "rgba8"), want)
    assert np.array_equal(CR.convert_ref(px[..., [2, 1, 0]], "bgr8"), want)
    assert np.array_equal(CR.convert_ref(px[..., [2, 1, 0, 3]], "bgra8"), want)
    assert not np.array_equal(CR.convert_ref(px[..., :3], "bgr8"), want)
    v = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(CR.convert_ref(v, "gray16", 8), v >> 8)
    assert np.array_equal(CR.convert_ref(v, "gray16", 4)[:4096], np.arange(4096) >> 4)
    assert (CR.convert_ref(v, "gray16", 4)[4096:] == 255).all() and (CR.convert_ref(v, "gray16", 0)[255:] == 255).all()


def test_anchor_committed_crop():
    z = np.load(os.path.join(GOLDEN, "convert_rgb_crop.npz"))
    rgb, (r, c) = z["rgb"], z["offset"]
    assert rgb.dtype == np.uint8 and rgb.shape == (192, 256, 3)
    assert os.path.getsize(os.path.join(GOLDEN, "convert_rgb_crop.npz")) <= 200 * 1024
    want = np.load(os.path.join(GOLDEN, "refimages.npz"))["image_1"][r:r + 192, c:c + 256]
    got = CR.convert_ref(rgb, "rgb8")
    assert np.array_equal(got, want)
    assert got.std() > 40 and not np.array_equal(CR.convert_ref(rgb, "bgr8"), want)  # textured, and colourful


# ---------------------------------------------------------------- svo_image_layout_bytes
def layout_bytes(fmt, width, height, count, shift=8, row_stride=0, image_stride=0):
    lay = _capi.SvoImageLayout(fmt, shift, row_stride, image_stride)
    n = ctypes.c_int64(-1)
    rc = _capi.lib().svo_image_layout_bytes(ctypes.byref(lay), width, height, count, ctypes.byref(n))
    return rc, n.value, _capi.lib().svo_last_error().decode()


@pytest.mark.parametrize("name", CR.FORMATS)
def test_layout_bytes_sizes(name):
    fmt, bpp = _capi.PIXEL_FORMATS[name], CR.BPP[name]
    assert _capi.PIXEL_SHAPES[name][0] == bpp
    for w, h, count in [(1, 1, 1), (67, 5, 1), (67, 5, 3), (1241, 376, 2)]:
        assert layout_bytes(fmt, w, h, count)[:2] == (0, w * h * bpp * count)
        rs = w * bpp + 6
        assert layout_bytes(fmt, w, h, count, row_stride=rs)[:2] == (0, rs * h * (count - 1) + rs * (h - 1) + w * bpp)
        ims = rs * (h + 5)
        got = layout_bytes(fmt, w, h, count, row_stride=rs, image_stride=ims)
        assert got[:2] == (0, ims * (count - 1) + rs * (h - 1) + w * bpp)
        assert got[1] == CR.layout_bytes(name, w, h, count, rs, ims)
        # the tightest strides: an image stride that ends with the last row's last pixel
        tight = rs * (h - 1) + w * bpp
        assert layout_bytes(fmt, w, h, count, row_stride=rs, image_stride=tight)[:2] == (0, tight * count)
    assert layout_bytes(fmt, 8, 8, 0)[:2] == (0, 0)


def test_layout_bytes_errors():
    G16, BGR = _capi.PIXEL_FORMATS["gray16"], _capi.PIXEL_FORMATS["bgr8"]
    cases = [(dict(fmt=6), "format"), (dict(fmt=-1), "format"),
             (dict(fmt=G16, shift=9), "shift"), (dict(fmt=G16, shift=-1), "shift"),
             (dict(fmt=BGR, row_stride=3 * 8 - 1), "row stride"),
             (dict(fmt=BGR, row_stride=30, image_stride=30 * 4 + 23), "image stride"),
             (dict(fmt=BGR, image_stride=24 * 5 - 1), "image stride"),
             (dict(fmt=G16, row_stride=17), "odd"), (dict(fmt=G16, row_stride=18, image_stride=18 * 5 + 1), "odd"),
             (dict(fmt=BGR, width=0), "size"), (dict(fmt=BGR, height=0), "size"), (dict(fmt=BGR, count=-1), "count")]
    for kw, word in cases:
        args = dict(fmt=0, width=8, height=5, count=2, shift=8, row_stride=0, image_stride=0)
        args.update(kw)
        rc, _, text = layout_bytes(**args)
        assert rc == _capi.SVO_ERR_ARG and word in text and "svo_image_layout_bytes" in text, (kw, rc, text)
    # a shift is read for GRAY16 alone
    assert layout_bytes(BGR, 8, 5, 1, shift=99)[0] == 0
    n = ctypes.c_int64()
    assert _capi.lib().svo_image_layout_bytes(None, 8, 5, 1, ctypes.byref(n)) == _capi.SVO_ERR_ARG
    assert b"null layout" in _capi.lib().svo_last_error()
    lay = _capi.SvoImageLayout(0, 0, 0, 0)
    assert _capi.lib().svo_image_layout_bytes(ctypes.byref(lay), 8, 5, 1, None) == _capi.SVO_ERR_ARG


def test_entry_points_validate_without_a_device():
    """The argument checks come before the device is touched: codes with texts on a machine without one."""
    L = _capi.lib()
    lay = _capi.SvoImageLayout(1, 0, 0, 0)
    buf = np.zeros(64, np.uint8)
    assert L.svo_convert_images(None, ctypes.byref(lay), 4, 4, 1, _capi.ptr(buf), _capi.ptr(buf)) == _capi.SVO_ERR_ARG
    assert b"null" in L.svo_last_error()
    assert L.svo_pyramid_set_upload_format(None, 0, 1, _capi.ptr(buf), ctypes.byref(lay), None) == _capi.SVO_ERR_ARG
    assert L.svo_pyramid_set_upload_format_device(None, 0, 1, _capi.ptr(buf), ctypes.byref(lay), None) == _capi.SVO_ERR_ARG
    assert b"svo_pyramid_set_upload_format_device" in L.svo_last_error()


# ---------------------------------------------------------------- the kernel's body on the CPU
def test_convert_model_runs_every_thread_of_the_launch(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "convert_model"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "convert_model.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ok, cases = r.stdout.split()
    # 5 byte formats x 11 widths x 3 heights x 4 row pads x 2 counts x 4 source x 4 output alignments, and GRAY16 with
    # 3 row pads and 2 source alignments
    assert ok == "ok" and int(cases) == 5 * 11 * 3 * 4 * 2 * 4 * 4 + 11 * 3 * 3 * 2 * 2 * 4


# ---------------------------------------------------------------- the mirrors
class Recorder:
    """Stands in for lib(): records the entry points called, every call returns SVO_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(core, "lib", lambda: rec)

    class Ctx:
        handle = ctypes.c_void_p(1)

        def synchronize(self):
            pass

    return rec, Ctx()


def names(rec):
    return [c[0] for c in rec.calls]


def test_default_calls_reach_the_existing_entry_points(recorder):
    rec, ctx = recorder
    ps = svo_amd.PyramidSet(2, 8, 4, 2, ctx)
    img = np.zeros((2, 4, 8), np.uint8)
    ps.upload(0, img)
    ps.upload(0, img, pixel_format="gray8", gray16_shift=3)
    ps.upload_device(0, 2, 4096)
    ps.upload_device(0, 2, 4096, pixel_format="gray8")
    svo_amd.Frame(svo_amd.PinholeCamera(8, 4, 10.0, 10.0, 4.0, 2.0), img[0], 2, ctx=ctx)
    assert names(rec) == ["svo_pyramid_set_create", "svo_pyramid_set_upload", "svo_pyramid_set_upload",
                          "svo_pyramid_set_upload_device", "svo_pyramid_set_upload_device",
                          "svo_pyramid_set_create", "svo_pyramid_set_upload", "svo_pyramid_set_build"]
    assert svo_amd.Config().pixel_format == "gray8" and svo_amd.Config().gray16_shift == 8
    ps.handle = None


def test_formats_reach_the_format_entry_points_with_their_layout(recorder):
    rec, ctx = recorder
    ps = svo_amd.PyramidSet(3, 8, 4, 2, ctx)
    big = np.zeros((3, 9, 16, 3), np.uint8)
    view = big[:, :4, :8]                       # rows and images at their own strides: passed through
    ps.upload(0, view, pixel_format="bgr8")
    ps.upload(1, big[0, :4, :8, ::-1], pixel_format="rgb8")   # reversed channels: made contiguous
    ps.upload(0, np.zeros((4, 8), np.uint16), pixel_format="gray16", gray16_shift=4)
    ps.upload_device(0, 3, 4096, pixel_format="gray8", row_stride=16)
    ps.upload_device(0, 3, 4096, pixel_format="bgra8", image_stride=999)
    got = [(n, a) for n, a in rec.calls if n != "svo_pyramid_set_create"]
    assert [n for n, _ in got] == ["svo_pyramid_set_upload_format"] * 3 + ["svo_pyramid_set_upload_format_device"] * 2

    def layout(args):
        lay = args[4]._obj
        return lay.format, lay.shift, lay.row_stride, lay.image_stride

    assert got[0][1][1:3] == (0, 3) and layout(got[0][1])[2:] == (48, 9 * 48) and layout(got[0][1])[0] == 1
    assert got[0][1][3].value == view.ctypes.data
    assert got[1][1][1:3] == (1, 1) and layout(got[1][1]) == (2, 8, 24, 96)
    assert layout(got[2][1]) == (5, 4, 16, 64)
    assert layout(got[3][1]) == (0, 8, 16, 0) and layout(got[4][1]) == (3, 8, 0, 999)
    assert all(a[5] is None for _, a in got)  # no camera: no map
    # 16-bit pixels at an odd address (a byte buffer cut one byte in): copied, so the pointer handed over is even
    odd = np.frombuffer(bytearray(4 * 8 * 2 + 1), np.uint8)[1:].view(np.uint16).reshape(4, 8)
    assert odd.ctypes.data % 2 == 1
    ps.upload(0, odd, pixel_format="gray16")
    assert rec.calls[-1][1][3].value % 2 == 0
    ps.handle = None


def test_shape_and_dtype_must_fit_the_format(recorder):
    rec, ctx = recorder
    ps = svo_amd.PyramidSet(1, 8, 4, 2, ctx)
    cam = svo_amd.PinholeCamera(8, 4, 10.0, 10.0, 4.0, 2.0)
    grey, colour, deep = np.zeros((4, 8), np.uint8), np.zeros((4, 8, 3), np.uint8), np.zeros((4, 8), np.uint16)
    bad = [(colour, "gray8"), (grey, "bgr8"), (grey, "rgb8"), (grey, "gray16"), (deep, "bgr8"), (colour, "bgra8"),
           (np.zeros((4, 8, 4), np.uint8), "rgb8"), (np.zeros((4, 8, 3), np.uint16), "bgr8"),
           (np.zeros((2, 2, 4, 8, 3), np.uint8), "bgr8"), (colour, "yuv"), (colour.astype(np.float32), "bgr8")]
    with pytest.raises(ValueError):
        ps.upload(0, np.zeros((4, 7, 3), np.uint8), pixel_format="bgr8")  # not the set's size
    for img, fmt in bad:
        with pytest.raises(ValueError):
            ps.upload(0, img, pixel_format=fmt)
        with pytest.raises(ValueError):
            svo_amd.ImagePyramid(img, 2, ctx, pixel_format=fmt)
        if fmt != "gray8":  # (with gray8 a Frame keeps the reference's own "Image Corrupted")
            with pytest.raises(ValueError):
                svo_amd.Frame(cam, img, 2, ctx=ctx, pixel_format=fmt)
    with pytest.raises(RuntimeError, match="Image Corrupted"):
        svo_amd.Frame(cam, colour, 2, ctx=ctx)
    with pytest.raises(ValueError):
        ps.upload_device(0, 1, 4096, pixel_format="yuv")
    with pytest.raises(ValueError):
        svo_amd.Frame(cam, np.zeros((5, 8, 3), np.uint8), 2, ctx=ctx, pixel_format="bgr8")  # not the camera's size
    assert names(rec) == ["svo_pyramid_set_create"]  # nothing reached the library
    with pytest.raises(TypeError):
        svo_amd.Config(pixel_fmt="bgr8")
    assert svo_amd.Config(pixel_format="rgb8", gray16_shift=4).pixel_format == "rgb8"
    ps.handle = None


# ---------------------------------------------------------------- the System test's scene
def test_scene_still_initialises_in_colour():
    """The condition of the GPU System test: on the grey images of the colour scene the restatement tracker still walks
    first -> second -> new and takes at least two keyframes after the second frame ((R, G, B) = (g, g, 255 - g); run
    here: keyframes at frames 0, 1, 4 and 7, closest decision margin 1.3e-4)."""
    rgb, _ = colour_scene()
    grey = CR.convert_ref(rgb, "rgb8")
    assert grey.std() > 0.7 * TS.sequence()[0].std()
    s, recs = SR.run(grey, SR.Config(**SC.config_kwargs()), False)
    assert [r["status"] for r in recs] == [SR.SECOND] + [SR.NEW] * 7
    assert all(r["result"] != SR.FAILED for r in recs)
    assert recs[1]["keyframes"] == 2 and recs[-1]["keyframes"] >= 4
    print({k: "%.2e" % v for k, v in s.margins.items()})
    assert min(s.margins.values()) >= SR.CAP, s.margins
