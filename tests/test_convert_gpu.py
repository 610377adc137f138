"""Pixel formats on the GPU (csrc/convert.hip behind svo_convert_images and svo_pyramid_set_upload_format[_device]):
every result bit-exact against the numpy restatement tests/convert_ref.py.

Edge shapes: widths 1, 2, 3, 4, 5, 7, 8, 9, 61, 64, 67 x heights 1, 2, 5 x row strides packed and packed + 1, 3, 13 bytes
(GRAY16: + 2, 6) x count 1 and 3 (count 3 with the image stride padded by 5 rows) x pointers offset by 0, 1, 2, 3 bytes
(GRAY16: 0, 2), every format.  All of them run through svo_convert_images (any size; the output planes of w * h bytes
start at every alignment).  A pyramid set is at least 3 x 3 pixels, so the two upload forms run the part of the list a
set can hold: widths >= 3 at height 5, host pointers and device pointers into a larger torch uint8 tensor, into
frames [1, 1 + count) of five, with the frames on either side and the padded input unchanged afterwards.  The shapes a set cannot hold reach the kernel only through svo_convert_images here; the
CPU model (tests/test_convert.py) runs them at every input and output alignment.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before libsvo_hip initialises HIP: torch's own HIP runtime then finds the GPU too)

import convert_ref as CR
import test_system as TS
import undistort_ref as U
from test_convert import GOLDEN, colour_scene
from test_undistort import LENSES, lib_camera, small_cam

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 61, 64, 67]
HEIGHTS = [1, 2, 5]
GUARD = 8  # bytes on either side of an input or output that must not change


def pads(fmt):
    return (0, 2, 6) if fmt == "gray16" else (0, 1, 3, 13)


def offsets(fmt):
    return (0, 2) if fmt == "gray16" else (0, 1, 2, 3)


def make_input(fmt, w, h, count, pad, off, seed):
    """(buffer, layout, images, grey): full-range random bytes (so the channels differ), the layout that starts `off`
    bytes into the buffer and ends GUARD bytes before its end, what it holds, and the restatement's result."""
    from svo_amd import _capi
    rs = w * CR.BPP[fmt] + pad
    ims = rs * (h + 5) if count > 1 else 0
    shift = seed % 9 if fmt == "gray16" else 8
    n = CR.layout_bytes(fmt, w, h, count, rs, ims)
    buf = np.random.default_rng(seed).integers(0, 256, off + n + GUARD, dtype=np.uint8)
    images = CR.from_bytes(buf[off:off + n], fmt, w, h, count, rs, ims)
    layout = _capi.SvoImageLayout(_capi.PIXEL_FORMATS[fmt], shift, rs if pad else 0, ims)
    return buf, layout, images, CR.convert_ref(images, fmt, shift)


def address(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("fmt", CR.FORMATS)
def test_convert_images_edge_shapes(fmt, w):
    import svo_amd
    from svo_amd import _capi
    ctx, L = svo_amd.default_context(), _capi.lib()
    seed = 0
    for h in HEIGHTS:
        for pad in pads(fmt):
            for count in (1, 3):
                for off in offsets(fmt):
                    seed += 1
                    buf, layout, _, want = make_input(fmt, w, h, count, pad, off, 100000 * w + seed)
                    before = buf.copy()
                    out = np.full(GUARD + want.size + GUARD, 0xA5, np.uint8)
                    _capi.check(L.svo_convert_images(ctx.handle, ctypes.byref(layout), w, h, count, address(buf, off),
                                                     address(out, GUARD)))
                    case = (h, pad, count, off)
                    assert np.array_equal(out[GUARD:-GUARD].reshape(want.shape), want), case
                    assert (out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all(), case
                    assert np.array_equal(buf, before), case


@pytest.mark.parametrize("w", [w for w in WIDTHS if w >= 3])
@pytest.mark.parametrize("fmt", CR.FORMATS)
def test_upload_format_edge_shapes(fmt, w):
    import svo_amd
    from svo_amd import _capi
    ctx, L = svo_amd.default_context(), _capi.lib()
    seed = 0
    for h in (5,):
        ps = svo_amd.PyramidSet(5, w, h, 1)
        state = np.random.default_rng(w + h).integers(0, 256, (5, h, w), dtype=np.uint8)
        ps.upload(0, state)
        for pad in pads(fmt):
            for count in (1, 3):
                for off in offsets(fmt):
                    for form in ("host", "device"):
                        seed += 1
                        buf, layout, _, want = make_input(fmt, w, h, count, pad, off, 200000 * w + seed)
                        case = (h, pad, count, off, form)
                        if form == "host":
                            before = buf.copy()
                            _capi.check(L.svo_pyramid_set_upload_format(ps.handle, 1, count, address(buf, off),
                                                                        ctypes.byref(layout), None))
                            ctx.synchronize()
                            assert np.array_equal(buf, before), case
                        else:
                            dev = torch.from_numpy(buf).cuda()
                            torch.cuda.synchronize()
                            ps.upload_device(1, count, dev.data_ptr() + off, pixel_format=fmt, gray16_shift=layout.shift,
                                             row_stride=layout.row_stride, image_stride=layout.image_stride)
                            ctx.synchronize()
                            assert np.array_equal(dev.cpu().numpy(), buf), case
                        state[1:1 + count] = want
                        for k in range(5):
                            assert np.array_equal(ps.download(k, 0), state[k]), case + (k,)
        ps.close()


def test_batch_spans_several_slices_of_the_grid():
    """Nine images: a thread walks four, so the grid has three slices, the last one short."""
    import svo_amd
    rng = np.random.default_rng(9)
    for fmt, shape, dtype in (("bgr8", (9, 5, 67, 3), np.uint8), ("gray16", (9, 5, 67), np.uint16)):
        imgs = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
        assert np.array_equal(svo_amd.convert_images(imgs, fmt, 3), CR.convert_ref(imgs, fmt, 3))


def test_exhaustive_colours():
    """One 4096 x 4096 RGB8 image holding all 2^24 colours."""
    import svo_amd
    v = np.arange(256, dtype=np.uint8)
    rgb = np.empty((256, 256, 256, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = v[:, None, None], v[None, :, None], v[None, None, :]
    rgb = rgb.reshape(4096, 4096, 3)
    ps = svo_amd.PyramidSet(1, 4096, 4096, 1)
    ps.upload(0, rgb, pixel_format="rgb8")
    assert np.array_equal(ps.download(0, 0), CR.convert_ref(rgb, "rgb8"))
    ps.upload(0, rgb, pixel_format="bgr8")
    assert np.array_equal(ps.download(0, 0), CR.convert_ref(rgb, "bgr8"))
    ps.close()


@pytest.mark.parametrize("shift", range(9))
def test_exhaustive_gray16(shift):
    import svo_amd
    v = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    ps = svo_amd.PyramidSet(1, 256, 256, 1)
    ps.upload(0, v, pixel_format="gray16", gray16_shift=shift)
    assert np.array_equal(ps.download(0, 0), CR.convert_ref(v, "gray16", shift))
    ps.close()


def test_committed_crop():
    import svo_amd
    z = np.load(os.path.join(GOLDEN, "convert_rgb_crop.npz"))
    rgb, (r, c) = z["rgb"], z["offset"]
    want = np.load(os.path.join(GOLDEN, "refimages.npz"))["image_1"][r:r + 192, c:c + 256]
    camera = svo_amd.PinholeCamera(256, 192, 200.0, 200.0, 128.0, 96.0)
    assert np.array_equal(svo_amd.Frame(camera, rgb, 2, pixel_format="rgb8").image_pyramid.get_base_image(), want)
    assert np.array_equal(svo_amd.convert_images(rgb, "rgb8"), want)


@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("fmt", ["bgr8", "gray16"])
@pytest.mark.parametrize("w,h", [(67, 5), (64, 64)])
def test_with_a_lens(w, h, fmt, lens):
    """Convert first, then remap: the result is remap_ref(convert_ref(raw)), from host and from device memory."""
    import svo_amd
    from svo_amd import _capi
    cam, d = small_cam(w, h), LENSES[lens]
    camera = lib_camera(cam, d)
    want_map = U.make_map(cam, d)
    buf, layout, _, grey = make_input(fmt, w, h, 3, 6, 2, 31 * w + h)
    want = np.stack([U.remap(g, *want_map) for g in grey])
    assert not np.array_equal(want, grey)
    old = np.random.default_rng(5).integers(0, 256, (5, h, w), dtype=np.uint8)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    for form in ("host", "device"):
        ps = svo_amd.PyramidSet(5, w, h, 1)
        ps.upload(0, old)
        if form == "host":
            _capi.check(_capi.lib().svo_pyramid_set_upload_format(ps.handle, 1, 3, address(buf, 2), ctypes.byref(layout),
                                                                  camera.undistort_map(ps.ctx).handle))
        else:
            ps.upload_device(1, 3, dev.data_ptr() + 2, camera, fmt, layout.shift, layout.row_stride, layout.image_stride)
        ps.ctx.synchronize()
        for k in range(5):
            assert np.array_equal(ps.download(k, 0), old[k] if k in (0, 4) else want[k - 1]), (form, k)
        ps.close()
    assert np.array_equal(dev.cpu().numpy(), buf)


def test_convert_images_round_trip():
    """Host to host through the Python mirror: a packed stack, a view with its own strides, one image."""
    import svo_amd
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (3, 40, 80, 4), dtype=np.uint8)
    view = big[:, 3:26, 5:72]
    for fmt in ("bgra8", "rgba8"):
        assert np.array_equal(svo_amd.convert_images(view, fmt), CR.convert_ref(view, fmt))
        assert np.array_equal(svo_amd.convert_images(np.ascontiguousarray(view), fmt), CR.convert_ref(view, fmt))
        assert np.array_equal(svo_amd.convert_images(view[1], fmt), CR.convert_ref(view[1], fmt))
    assert np.array_equal(svo_amd.convert_images(view[..., :3][..., ::-1], "rgb8"), CR.convert_ref(view[..., :3], "bgr8"))
    grey = big[..., 0]  # pixels 4 bytes apart: made contiguous
    assert np.array_equal(svo_amd.convert_images(grey, "gray8"), grey)
    deep = rng.integers(0, 65536, (2, 23, 67)).astype(np.uint16)
    assert np.array_equal(svo_amd.convert_images(deep[:, :, 1:60], "gray16", 4), CR.convert_ref(deep[:, :, 1:60], "gray16", 4))


def test_errors_are_codes_with_text():
    import svo_amd
    from svo_amd import _capi
    L = _capi.lib()
    ps = svo_amd.PyramidSet(2, 37, 23, 1)
    img = np.zeros((23, 37, 3), np.uint8)
    lay = _capi.SvoImageLayout(_capi.PIXEL_FORMATS["bgr8"], 8, 0, 0)
    other_size = svo_amd.UndistortMap(lib_camera(small_cam(64, 48), LENSES["mixed"]))
    assert L.svo_pyramid_set_upload_format(ps.handle, 0, 1, address(img), ctypes.byref(lay), other_size.handle) == _capi.SVO_ERR_ARG
    text = L.svo_last_error().decode()
    assert "64x48" in text and "37x23" in text
    ctx2 = svo_amd.Context(0)
    other_ctx = svo_amd.UndistortMap(lib_camera(small_cam(37, 23), LENSES["mixed"]), ctx2)
    assert L.svo_pyramid_set_upload_format(ps.handle, 0, 1, address(img), ctypes.byref(lay), other_ctx.handle) == _capi.SVO_ERR_ARG
    assert "another context" in L.svo_last_error().decode()
    other_ctx.close()
    ctx2.close()
    assert L.svo_pyramid_set_upload_format(ps.handle, 0, 1, address(img), None, None) == _capi.SVO_ERR_ARG
    assert "null layout" in L.svo_last_error().decode()
    g16 = _capi.SvoImageLayout(_capi.PIXEL_FORMATS["gray16"], 8, 0, 0)
    deep = np.zeros(23 * 37 * 2 + 2, np.uint8)
    dev = torch.zeros(23 * 37 * 2 + 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.svo_pyramid_set_upload_format(ps.handle, 0, 1, address(deep, 1), ctypes.byref(g16), None) == _capi.SVO_ERR_ARG
    assert "odd" in L.svo_last_error().decode()
    assert L.svo_pyramid_set_upload_format_device(ps.handle, 0, 1, ctypes.c_void_p(dev.data_ptr() + 1), ctypes.byref(g16),
                                                  None) == _capi.SVO_ERR_ARG
    assert "odd" in L.svo_last_error().decode()
    out = np.zeros(23 * 37, np.uint8)
    assert L.svo_convert_images(ps.ctx.handle, ctypes.byref(g16), 37, 23, 1, address(deep, 1), address(out)) == _capi.SVO_ERR_ARG
    assert "odd" in L.svo_last_error().decode()
    assert L.svo_pyramid_set_upload_format(ps.handle, 1, 2, address(img), ctypes.byref(lay), None) == _capi.SVO_ERR_ARG
    assert "out of range" in L.svo_last_error().decode()
    with pytest.raises(svo_amd.SvoError) as e:
        ps.upload_device(0, 1, dev.data_ptr(), pixel_format="bgr8", row_stride=37 * 3 - 1)
    assert e.value.code == _capi.SVO_ERR_ARG and "row stride" in str(e.value)
    ps.close()


def test_mirror_formats_give_their_own_grey():
    import svo_amd
    w, h = 67, 23
    img = np.random.default_rng(4).integers(0, 256, (h, w, 3), dtype=np.uint8)
    camera = svo_amd.PinholeCamera(w, h, 40.0, 40.0, 33.0, 11.0)
    bgr = svo_amd.Frame(camera, img, 2, pixel_format="bgr8").image_pyramid
    rgb = svo_amd.Frame(camera, img, 2, pixel_format="rgb8").image_pyramid
    assert np.array_equal(bgr.get_base_image(), CR.convert_ref(img, "bgr8"))
    assert np.array_equal(rgb.get_base_image(), CR.convert_ref(img, "rgb8"))
    assert not np.array_equal(bgr.get_base_image(), rgb.get_base_image())
    # the levels above are those of the grey image uploaded the old way
    plain = svo_amd.ImagePyramid(CR.convert_ref(img, "rgb8"), 2)
    assert np.array_equal(rgb.get_image_at_level(1), plain.get_image_at_level(1))
    assert np.array_equal(rgb.get_gradient_at_level(0), plain.get_gradient_at_level(0))
    deep = np.random.default_rng(5).integers(0, 4096, (h, w)).astype(np.uint16)
    got = svo_amd.ImagePyramid(deep, 2, pixel_format="gray16", gray16_shift=4).get_base_image()
    assert np.array_equal(got, CR.convert_ref(deep, "gray16", 4))


def equal_runs(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in TS.EXACT:
            assert g[name] == w[name], (k, name, g[name], w[name])
        assert np.asarray(g["pose"], np.float64).tobytes() == np.asarray(w["pose"], np.float64).tobytes(), (k, g["pose"], w["pose"])


def test_system_in_colour_is_the_system_on_the_grey_frames():
    """System(Config(pixel_format="rgb8")) on the colour scene against System on convert_ref of those frames: every
    per-frame record and the trajectory text, in every bit."""
    rgb, _ = colour_scene()
    system, recs, text = TS.gpu_run(rgb, pixel_format="rgb8")
    grey = CR.convert_ref(rgb, "rgb8")
    assert np.array_equal(system.cur_frame.image_pyramid.get_base_image(), grey[-1])
    _, want, want_text = TS.gpu_run(grey)
    equal_runs(recs, want)
    assert text == want_text and text.count("\n") == len(rgb)
    assert [r["keyframes"] for r in recs][1] == 2 and recs[-1]["keyframes"] >= 4


def test_system_in_colour_cpp_mirror_matches_python_mirror(tmp_path):
    import svo_amd.synth as synth
    rgb, _ = colour_scene()
    system, want, text = TS.gpu_run(rgb, pixel_format="rgb8")
    data, images = synth.write_system_problem(system.config, rgb, system.map.cell_orders, tmp_path)
    assert os.path.getsize(images) == rgb.size
    out = subprocess.run([TS.HOST_CHECK, "system", data, images], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got, trajectory, _ = TS.parse_host_system(out.stdout)
    equal_runs(got, want)
    assert trajectory == text
