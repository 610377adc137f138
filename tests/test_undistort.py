"""Lens undistortion ahead of the pyramid (contract: include/svo_c.h, svo_undistort_*; restatement: tests/undistort_ref.py).

CPU (not gpu)
  anchor: the restatement on the green channel of the reference's tests/test_data/camera/undistort_input.png against the
  recorded cv::remap result undistort_ref.png (tests/golden/undistort_ref.npz, camera of tests/test_camera.cpp:107-111).
  Measured: 47 of 1 228 800 bytes differ, by at most 3 grey levels, every one at a pixel whose u * 32 or v * 32 lies
  within 0.0019 of a rounding tie (there the recording sits one 1/32-pixel map step from the fp64 map).  Asserted: tie
  distance <= 0.005, difference <= 3, at most 0.01 % of the channel (122 bytes).
  point helpers: undistorted_pixel(raw_pixel(p)) = p within 1e-9 px over the fixture camera's image (measured 9.1e-13
  with the contract's 40 iterations; 20 iterations leave 1.2e-5 and 30 leave 3.0e-9 at the corners, which is why the
  contract says 40); the library's scalar helpers equal the restatement's in every bit, and the C++ mirror's equal
  the Python mirror's (build/svo_host_check undistort_points).

GPU: the device map equals the restatement's in every entry, the remap in every byte: the fixture channel, random
images at 37x23, 64x48, 5x3 and 1x1, k1 = +-0.8 at fx = w/2 (taps leave the image on all four sides, X = -1 and Y = -1
half-in taps, whole regions 0: each asserted on the restatement first), a purely tangential lens, batches that start
off a dword boundary and that span more than one slice of the grid, frames [1, 4) of a five-frame set with its
neighbours untouched, and upload_undistort + build against upload(restatement) + build on every level of both stacks.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before libsvo_hip initialises HIP: torch's own HIP runtime then finds the GPU too)

import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "svo_host_check")
SIZES = [(37, 23), (64, 48), (5, 3), (1, 1), (1, 7), (2, 3)]  # a one-column image takes a kernel of its own
LENSES = {"k1+": (0.8, 0, 0, 0, 0), "k1-": (-0.8, 0, 0, 0, 0), "tangential": (0, 0, 0.05, 0, 0),
          "mixed": (-0.23, 0.06, 0.01, -0.02, -0.0075)}


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "undistort_ref.npz"))
    c = z["camera"]
    cam = dict(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), width=int(c[4]), height=int(c[5]))
    out = dict(cam=cam, d=tuple(float(v) for v in z["dist"]), input=z["input_g"], ref=z["ref_g"])
    for k in ("input", "ref"):
        out[k].flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def fixture_restated():
    f = fixture()
    m = U.make_map(f["cam"], f["d"])
    out = U.remap(f["input"], *m)
    for a in m + (out,):
        a.flags.writeable = False
    return m, out


def small_cam(w, h):
    """fx = fy = w / 2 (the image spans x in about [-1, 1]), the principal point off the centre and off the grid."""
    return dict(fx=w / 2.0, fy=w / 2.0, cx=(w - 1) / 2.0 + 0.3, cy=(h - 1) / 2.0 - 0.2, width=w, height=h)


def lib_camera(cam, d):
    import svo_amd
    return svo_amd.PinholeCamera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], *d)


def random_image(w, h, seed=0, count=None):
    rng = np.random.default_rng(1000 * w + h + seed)
    return rng.integers(0, 256, size=(h, w) if count is None else (count, h, w), dtype=np.uint8)


# ---------------------------------------------------------------- CPU
def test_anchor_recorded_opencv_result():
    f = fixture()
    _, out = fixture_restated()
    diff = np.abs(out.astype(np.int32) - f["ref"].astype(np.int32))
    ii, jj = np.nonzero(diff)
    print("differing bytes: %d of %d, largest difference %d" % (len(ii), diff.size, int(diff.max())))
    u, v = U.raw_uv(f["cam"], f["d"])
    cam = lib_camera(f["cam"], f["d"])
    worst = 0.0
    for i, j in zip(ii, jj):
        r = cam.raw_pixel((j, i))  # the library's helper is the contract's (u, v), in every bit
        assert r[0] == u[i, j] and r[1] == v[i, j]
        tie = min(abs(t - np.floor(t) - 0.5) for t in (r[0] * 32.0, r[1] * 32.0))
        worst = max(worst, tie)
    print("largest distance of a differing pixel from a rounding tie: %.6f" % worst)
    assert worst <= 0.005
    assert diff.max() <= 3
    assert len(ii) <= 122  # 0.01 % of 1 228 800


def test_point_helpers_round_trip():
    import svo_amd
    f = fixture()
    cam = lib_camera(f["cam"], f["d"])
    assert svo_amd.UNDISTORT_POINT_ITERATIONS == U.ITERATIONS
    w, h = f["cam"]["width"], f["cam"]["height"]
    worst = 0.0
    for j in np.linspace(0.0, w - 1.0, 41):
        for i in np.linspace(0.0, h - 1.0, 31):
            raw = cam.raw_pixel((j, i))
            back = cam.undistorted_pixel(raw)
            assert tuple(raw) == U.raw_pixel(f["cam"], f["d"], (j, i))
            assert tuple(back) == U.undistorted_pixel(f["cam"], f["d"], raw)
            worst = max(worst, abs(back[0] - j), abs(back[1] - i))
    print("largest round-trip error: %.3e px" % worst)
    assert worst <= 1e-9
    # the vectorised restatement (the distorted test scene is made with it) is the scalar one, elementwise
    pts = np.array([[3.0, 5.0], [w - 1.0, h - 1.0], [640.25, 17.5]])
    vec = U.undistorted_pixels(f["cam"], f["d"], pts)
    assert all(tuple(vec[k]) == U.undistorted_pixel(f["cam"], f["d"], pts[k]) for k in range(len(pts)))


def test_point_helpers_cpp_mirror_equals_python_mirror(tmp_path):
    f = fixture()
    cases = [(f["cam"], f["d"])] + [(small_cam(64, 48), LENSES[k]) for k in ("tangential", "mixed")]
    rng = np.random.default_rng(3)
    for n, (c, d) in enumerate(cases):
        pts = np.stack([rng.uniform(0, c["width"] - 1, 64), rng.uniform(0, c["height"] - 1, 64)], axis=1)
        data = tmp_path / ("points%d.bin" % n)
        np.concatenate([[c["fx"], c["fy"], c["cx"], c["cy"], c["width"], c["height"]], d, [len(pts)],
                        pts.ravel()]).astype(np.float64).tofile(data)
        out = subprocess.run([HOST_CHECK, "undistort_points", str(data)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        got = np.array([[float.fromhex(x) for x in line.split()[1:]] for line in out.stdout.splitlines()])
        cam = lib_camera(c, d)
        want = np.array([np.concatenate([cam.raw_pixel(p), cam.undistorted_pixel(cam.raw_pixel(p))]) for p in pts])
        assert got.tobytes() == want.tobytes()


def test_camera_defaults_stay_the_plain_pinhole():
    import svo_amd
    cam = svo_amd.PinholeCamera.kitti()
    assert cam.d == (0.0,) * 5 and not cam.apply_distortion
    assert svo_amd.PinholeCamera(64, 48, 32, 32, 31, 23, 0, 0, 0.05).apply_distortion  # tangential alone applies
    img = random_image(1241, 376)
    out = cam.undistort_image(img)  # a copy, and nothing of the device is touched (no context on this path)
    assert out is not img and np.array_equal(out, img) and not cam._maps
    assert all(getattr(svo_amd.Config(), "d%d" % k) == 0.0 for k in range(5))
    p = cam.raw_pixel((100.0, 50.0))
    assert abs(p[0] - 100.0) < 1e-12 and abs(p[1] - 50.0) < 1e-12


def test_strong_lens_cases_reach_every_border_path():
    """What the GPU remap cases below rely on, asserted on the restatement."""
    w, h = 64, 48
    X, Y, ax, ay = (a.astype(np.int32) for a in U.make_map(small_cam(w, h), LENSES["k1+"]))
    assert (X < -1).any() and (X >= w).any() and (Y < -1).any() and (Y >= h).any()       # out on all four sides
    inside_rows, inside_cols = (Y >= 0) & (Y < h - 1), (X >= 0) & (X < w - 1)
    assert ((X == -1) & inside_rows & (ax > 0)).any() and ((Y == -1) & inside_cols & (ay > 0)).any()  # half in
    assert ((X == w - 1) & inside_rows).any() and ((Y == h - 1) & inside_cols).any()
    out = U.remap(random_image(w, h) | 1, X, Y, ax, ay)                                  # no zero byte in the input
    assert (out[0] == 0).all() and (out[-1] == 0).all() and (out[:, 0] == 0).all() and (out[:, -1] == 0).all()
    assert (out != 0).any()
    Xn, Yn, _, _ = U.make_map(small_cam(w, h), LENSES["k1-"])
    assert (Xn >= 0).all() and (Xn < w).all() and (Yn >= 0).all() and (Yn < h).all()     # the barrel case stays inside
    Xt, Yt, axt, ayt = U.make_map(small_cam(w, h), LENSES["tangential"])
    assert (axt != 0).any() and (Yt != np.arange(h)[:, None]).any()                      # the tangential map is no identity


# ---------------------------------------------------------------- GPU
def gpu_map(cam, d):
    import svo_amd
    return svo_amd.UndistortMap(lib_camera(cam, d))


def check_map(m, want):
    xy, frac = m.download()
    X, Y, ax, ay = want
    assert np.array_equal(xy[..., 0], X) and np.array_equal(xy[..., 1], Y)
    assert np.array_equal(frac, U.pack_frac(ax, ay))


@pytest.mark.gpu
def test_gpu_fixture_map_and_remap():
    f = fixture()
    want_map, want = fixture_restated()
    m = gpu_map(f["cam"], f["d"])
    check_map(m, want_map)
    assert np.array_equal(m.undistort(f["input"]), want)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_small_maps_and_remaps(w, h, lens):
    cam, d = small_cam(w, h), LENSES[lens]
    want_map = U.make_map(cam, d)
    m = gpu_map(cam, d)
    check_map(m, want_map)
    img = random_image(w, h)
    assert np.array_equal(m.undistort(img), U.remap(img, *want_map))
    # three planes of w * h bytes: the second and third start off a dword boundary when w * h is odd; eleven planes
    # span two slices of the grid (a thread walks eight images with its map entries)
    for count in (3, 11):
        imgs = random_image(w, h, seed=count, count=count)
        got = m.undistort(imgs)
        for k in range(count):
            assert np.array_equal(got[k], U.remap(imgs[k], *want_map)), (count, k)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,lens", [(37, 23, "k1+"), (64, 48, "mixed")])
def test_gpu_upload_undistort_into_a_set(w, h, lens):
    """count = 3 at first = 1 into five frames: the neighbours stay, and the pyramids built on top equal those of the
    restatement's output uploaded the old way, on every level of both stacks; host and device sources agree."""
    import svo_amd
    cam, d = small_cam(w, h), LENSES[lens]
    camera = lib_camera(cam, d)
    want_map = U.make_map(cam, d)
    levels = 3
    old = random_image(w, h, seed=7, count=5)
    raw = random_image(w, h, seed=8, count=3)
    want = np.stack([U.remap(r, *want_map) for r in raw])
    ref = svo_amd.PyramidSet(5, w, h, levels)
    ref.upload(0, old)
    ref.upload(1, want)
    ref.build()
    dev = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    for source in ("host", "device"):
        s = svo_amd.PyramidSet(5, w, h, levels)
        s.upload(0, old)
        if source == "host":
            s.upload(1, raw, camera)
        else:
            s.upload_device(1, 3, dev.data_ptr(), camera)
        for k in range(5):
            assert np.array_equal(s.download(k, 0), old[k] if k in (0, 4) else want[k - 1]), (source, k)
        s.build()
        for k in range(5):
            for level in range(levels):
                for grad in (False, True):
                    assert np.array_equal(s.download(k, level, grad), ref.download(k, level, grad)), (source, k, level, grad)
        s.ctx.synchronize()
        s.close()


@pytest.mark.gpu
def test_gpu_zero_coefficients_are_todays_path():
    import svo_amd
    w, h = 64, 48
    img = random_image(w, h, seed=2)
    plain = svo_amd.PinholeCamera(w, h, 32.0, 32.0, 31.0, 23.0)
    zero = svo_amd.PinholeCamera(w, h, 32.0, 32.0, 31.0, 23.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    a, b = svo_amd.Frame(plain, img, 3), svo_amd.Frame(zero, img, 3)
    for level in range(3):
        assert np.array_equal(a.image_pyramid.get_image_at_level(level), b.image_pyramid.get_image_at_level(level))
        assert np.array_equal(a.image_pyramid.get_gradient_at_level(level), b.image_pyramid.get_gradient_at_level(level))
    assert np.array_equal(b.image_pyramid.get_base_image(), img)
    out = zero.undistort_image(img)
    assert out is not img and np.array_equal(out, img) and not zero._maps  # no map was ever made
    lens = svo_amd.PinholeCamera(w, h, 32.0, 32.0, 31.0, 23.0, *LENSES["mixed"])
    want = U.undistort(img, dict(fx=32.0, fy=32.0, cx=31.0, cy=23.0, width=w, height=h), LENSES["mixed"])
    assert np.array_equal(svo_amd.Frame(lens, img, 3).image_pyramid.get_base_image(), want)
    assert np.array_equal(lens.undistort_image(img), want)


@pytest.mark.gpu
def test_gpu_errors_are_codes_with_text():
    import svo_amd
    from svo_amd import _capi
    m = gpu_map(small_cam(64, 48), LENSES["mixed"])
    s = svo_amd.PyramidSet(2, 37, 23, 2)
    with pytest.raises(svo_amd.SvoError) as e:
        _capi.check(_capi.lib().svo_pyramid_set_upload_undistort(s.handle, 0, 1, _capi.ptr(random_image(37, 23)), m.handle))
    assert e.value.code == _capi.SVO_ERR_ARG and "64x48" in str(e.value) and "37x23" in str(e.value)
    for w, h in ((32768, 4), (4, 40000)):
        with pytest.raises(svo_amd.SvoError) as e:
            svo_amd.UndistortMap(svo_amd.PinholeCamera(w, h, 100.0, 100.0, 2.0, 2.0, 0.1))
        assert e.value.code == _capi.SVO_ERR_ARG and "int16" in str(e.value)
