"""svo_klt_track (pyramidal Lucas-Kanade, include/svo_c.h "sparse optical flow") against the numpy restatement of
its contract (tests/klt_ref.py), the restatement against scenes of known flow, and the frame-level mirrors of
algorithm::computeOpticalFlowSparse (Python and C++)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import klt_ref as K
import svo_amd
from svo_amd import _capi, _paths

TRUTH_SHIFTS = [(0.0, 0.0), (0.37, -0.81), (3.3, -2.6), (7.25, 4.5), (12.6, -9.2), (20.5, 3.0)]
# the largest error of the restatement over the truth scenes below (measured by test_restatement_tracks_known_shifts,
# which prints it): the bound of that test is twice this
TRUTH_MAX_ERR = 0.050


def _truth_scene(shift, seed=5):
    w, h = 320, 240
    tex = K.Texture(seed)
    ref, cur = tex.render(w, h), tex.render(w, h, shift)
    ys, xs = np.mgrid[14:h - 14:17, 13:w - 13:19].astype(np.float64)
    px = np.stack([xs.ravel() + 0.29, ys.ravel() + 0.63], axis=1)
    true = px + np.asarray(shift)
    inside = ((px >= 12).all(axis=1) & (px[:, 0] <= w - 1 - 12) & (px[:, 1] <= h - 1 - 12) & (true >= 12).all(axis=1) &
              (true[:, 0] <= w - 1 - 12) & (true[:, 1] <= h - 1 - 12))
    return K.pyramid_levels(ref, 4), K.pyramid_levels(cur, 4), px[inside], true[inside]


def test_restatement_tracks_known_shifts():
    """Band-limited 320 x 240 textures shifted by TRUTH_SHIFTS, window 11, 4 levels: every point whose reference and
    true positions lie >= 12 px inside is tracked, to within 2 x TRUTH_MAX_ERR.  Measured largest error of the
    restatement over these scenes: 0.0498 px, at shift (3.3, -2.6) (the factor 2 allows for texture-seed variation)."""
    worst = 0.0
    for shift in TRUTH_SHIFTS:
        rp, cp, px, true = _truth_scene(shift)
        assert len(px) > 100
        cur, status, trace, _ = K.klt_track(rp, cp, px, px, 11, 3, 30, 1e-4, 1e-4)
        err = np.linalg.norm(cur - true, axis=1)
        print(f"shift {shift}: {len(px)} points, tracked {int(status.sum())}, max error {err.max():.4f} px")
        assert status.all()
        worst = max(worst, float(err.max()))
    print(f"largest error over the truth scenes: {worst:.4f} px")
    assert worst <= 2 * TRUTH_MAX_ERR


def test_restatement_zero_shift_is_a_fixed_point():
    rp, cp, px, _ = _truth_scene((0.0, 0.0))
    cur, status, trace, _ = K.klt_track(rp, cp, px, px, 11, 3, 30, 1e-4, 1e-4)
    assert status.all()
    assert np.array_equal(cur, px.astype(np.float32).astype(np.float64))
    assert (trace[:, :, 0] == 1).all() and (trace[:, :, 1] == K.EPS).all()


# ---------------------------------------------------------------- coverage of the committed GPU scenes (CPU)
def test_gpu_scenes_have_no_borderline_point():
    for name in K.GPU_SCENES:
        assert not K.gpu_scene_reference(name)[3].any(), name


def test_gpu_scenes_reach_every_exit():
    seen = set()
    for name in K.GPU_SCENES:
        seen |= set(np.unique(K.gpu_scene_reference(name)[2][:, :, 1]).tolist())
    for code in range(1, 7):
        assert code in seen, code
    assert K.ITERATION_LIMIT in np.unique(K.gpu_scene_reference("iter2")[2][:, :, 1])


@pytest.mark.parametrize("name", ["win5", "win11", "win21"])
def test_gpu_scenes_cover_edges_outside_and_rectangle(name):
    s = K.gpu_scene(name)
    _, status, trace, _ = K.gpu_scene_reference(name)
    px = s["ref_px"].astype(np.float32).astype(np.float64)
    win, h = s["win"], (s["win"] - 1) // 2
    H, W = s["ref_img"].shape
    ran = trace[:, 0, 1] != K.TEMPLATE_OUT  # the level-0 template was formed
    lo, hi = np.floor(px - h), np.floor(px - h) + win  # first and last column / row a window reads
    for crossing in (lo[:, 0] < 0, hi[:, 0] > W - 1, lo[:, 1] < 0, hi[:, 1] > H - 1):
        assert (crossing & ran).any()
    outside = (px[:, 0] < -win) | (px[:, 1] < -win) | (px[:, 0] > W - 1 + win) | (px[:, 1] > H - 1 + win)
    assert outside.any() and (trace[outside, 0, 1] == K.TEMPLATE_OUT).all() and not status[outside].any()
    x0, y0, rw, rh = K.RECT
    assert rw >= 40 and rh >= 40 and (s["ref_img"][y0:y0 + rh, x0:x0 + rw] == s["ref_img"][y0, x0]).all()
    in_rect = (lo[:, 0] >= x0 + 1) & (hi[:, 0] + 1 <= x0 + rw - 2) & (lo[:, 1] >= y0 + 1) & (hi[:, 1] + 1 <= y0 + rh - 2)
    assert in_rect.any() and (trace[in_rect, 0, 1] == K.MIN_EIG).all() and not status[in_rect].any()


def test_gpu_scene_cut_uses_the_level_cut_rule():
    s = K.gpu_scene("cut")
    shapes = [p.shape for p in K.pyramid_levels(s["ref_img"], 4)]
    assert shapes[3] == (8, 12) and K.top_level(shapes, s["win"], 3) == 2
    trace = K.gpu_scene_reference("cut")[2]
    assert (trace[:, 3] == 0).all() and (trace[:, 2, 1] != K.SKIPPED).all()
    full = K.gpu_scene("win11")
    assert K.top_level([p.shape for p in K.pyramid_levels(full["ref_img"], 4)], 11, 3) == 3


# ---------------------------------------------------------------- C ABI (no device)
def test_abi_exports_klt_track_with_the_documented_signature():
    assert "svo_klt_track" in _capi.EXPORTED
    fn = _capi.lib().svo_klt_track
    c_void_p, c_int32, c_double = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert fn.restype is c_int32
    assert list(fn.argtypes) == [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                 c_int32, c_int32, c_double, c_double, c_void_p, c_void_p, c_void_p]
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo_c.h")).read()
    decl = src[src.index("int svo_klt_track("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int svo_klt_track(svo_ctx* ctx, const svo_pyramid_set* ref_set, const svo_pyramid_set* cur_set, "
                    "int32_t n_pairs, const int32_t* frames, const int32_t* feat_off, const double* ref_px, "
                    "double* cur_px, int32_t win, int32_t max_level, int32_t max_iterations, double epsilon, "
                    "double min_eig_threshold, uint8_t* status, int32_t* trace, double* median_disparity)")
    assert _capi.lib().svo_abi_version() == 2


@pytest.mark.parametrize("win,max_level,what", [(10, 3, b"win"), (2, 3, b"win"), (1, 3, b"win"), (23, 3, b"win"),
                                                (11, -1, b"max_level")])
def test_abi_rejects_scalar_arguments_before_any_device_work(win, max_level, what):
    """An even window, one below 3 or above 21 and a negative max_level are SVO_ERR_ARG before the context or a set
    is looked at (all of them NULL here; no device exists on this path)."""
    L = _capi.lib()
    assert L.svo_klt_track(None, None, None, 0, None, None, None, None, win, max_level, 30, 1e-4, 1e-4, None, None,
                           None) == _capi.SVO_ERR_ARG
    assert what in L.svo_last_error()


def test_abi_rejects_null_handles():
    off = np.zeros(1, np.int32)
    L = _capi.lib()
    assert L.svo_klt_track(None, None, None, 0, None, _capi.ptr(off), None, None, 11, 3, 30, 1e-4, 1e-4, None, None,
                           None) == _capi.SVO_ERR_ARG
    assert b"null" in L.svo_last_error()


# ---------------------------------------------------------------- GPU
def _sets(images_ref, images_cur, levels=4):
    h, w = images_ref[0].shape
    out = []
    for imgs in (images_ref, images_cur):
        s = svo_amd.PyramidSet(len(imgs), w, h, levels)
        s.upload(0, np.stack(imgs))
        s.build()
        out.append(s)
    return out


def _run_scene(name, count=None, **kw):
    s = K.gpu_scene(name)
    n = len(s["ref_px"]) if count is None else count
    rs, cs = _sets([s["ref_img"]], [s["cur_img"]])
    got = svo_amd.klt_track_batch(rs, cs, [[0, 0]], [0, n], s["ref_px"][:n], s["init"][:n], s["win"], s["max_level"],
                                  s["max_iterations"], 1e-4, 1e-4, trace=True, **kw)
    return got, [a[:n] for a in K.gpu_scene_reference(name)]


def _assert_equal(got, want):
    cur, status, _, trace = got
    assert np.array_equal(status, want[1])
    assert np.array_equal(trace, want[2])
    assert cur.tobytes() == want[0].tobytes()  # bit-equal positions, every point


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["win5", "win11", "win21", "iter2", "cut"])
def test_gpu_matches_restatement(name):
    got, want = _run_scene(name)
    _assert_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_gpu_point_counts(count):
    got, want = _run_scene("win11", count)
    assert len(got[0]) == count
    _assert_equal(got, want)


def _batch():
    a, b = K.gpu_scene("win11"), K.gpu_scene("noisy")
    na, nb = 100, len(b["ref_px"])
    rs, cs = _sets([a["ref_img"], b["ref_img"]], [a["cur_img"], b["cur_img"]])
    off = [0, na, na, na + nb]
    ref_px = np.concatenate([a["ref_px"][:na], b["ref_px"]])
    init = np.concatenate([a["init"][:na], b["init"]])
    return rs, cs, [[0, 0], [1, 0], [1, 1]], off, ref_px, init


@pytest.mark.gpu
def test_gpu_batch_of_unequal_pairs():
    rs, cs, frames, off, ref_px, init = _batch()
    got = svo_amd.klt_track_batch(rs, cs, frames, off, ref_px, init, 11, 3, 30, 1e-4, 1e-4, trace=True)
    want = [np.concatenate([x[:100], y]) for x, y in zip(K.gpu_scene_reference("win11"), K.gpu_scene_reference("noisy"))]
    _assert_equal(got, want)
    assert want[1][100:].sum() > 40  # the noisy start is tracked, not merely rejected
    # median_disparity: computeMedian of the tracked points' float32 differences; NaN for the empty pair
    med = got[2]
    assert np.isnan(med[1])
    for p, (lo, hi) in enumerate([(0, 100), (100, 100), (100, len(ref_px))]):
        if lo == hi:
            continue
        t = want[1][lo:hi] == 1
        d32 = ref_px[lo:hi][t].astype(np.float32) - want[0][lo:hi][t].astype(np.float32)
        d = d32.astype(np.float64)
        disp = np.sort(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
        m = len(disp) // 2  # the two middle order statistics (distinct values: nth_element leaves them there)
        assert med[p] == (disp[m] if len(disp) % 2 else (disp[m - 1] + disp[m]) / 2.0)


@pytest.mark.gpu
def test_gpu_two_runs_give_equal_bytes():
    rs, cs, frames, off, ref_px, init = _batch()
    one = svo_amd.klt_track_batch(rs, cs, frames, off, ref_px, init, 11, 3, 30, 1e-4, 1e-4, trace=True)
    two = svo_amd.klt_track_batch(rs, cs, frames, off, ref_px, init, 11, 3, 30, 1e-4, 1e-4, trace=True)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_gpu_rejects_arguments_that_need_a_context():
    s = K.gpu_scene("cut")
    rs, cs = _sets([s["ref_img"]], [s["cur_img"]])
    other = svo_amd.PyramidSet(1, 160, 120, 4)
    px = s["ref_px"][:4]

    def code(ref_set, cur_set, frames, max_level):
        with pytest.raises(svo_amd.SvoError) as e:
            svo_amd.klt_track_batch(ref_set, cur_set, frames, [0, 4], px, px, 11, max_level)
        return e.value.code
    assert code(rs, cs, [[0, 0]], 4) == _capi.SVO_ERR_ARG       # max_level >= the sets' level count
    assert code(rs, other, [[0, 0]], 3) == _capi.SVO_ERR_ARG    # mismatched geometry
    assert code(rs, cs, [[1, 0]], 3) == _capi.SVO_ERR_ARG       # frame index out of range
    assert code(rs, cs, [[0, -1]], 3) == _capi.SVO_ERR_ARG
    svo_amd.klt_track_batch(rs, cs, [[0, 0]], [0, 4], px, px, 11, 3)


# ---------------------------------------------------------------- frame level
def _frame_pair(n=None):
    s = K.gpu_scene("win11")
    cam = svo_amd.PinholeCamera(160, 120, 150.0, 150.0, 80.0, 60.0)
    ref = svo_amd.Frame(cam, s["ref_img"], 4)
    cur = svo_amd.Frame(cam, s["cur_img"], 4)
    px = s["ref_px"] if n is None else s["ref_px"][:n]
    ref.features = svo_amd.Feature._many(ref, px)
    return ref, cur, px


def _frame_reference(px):
    """What the tracker gives for the frame call: initial flow = the reference positions."""
    s = K.gpu_scene("win11")
    rp, cp = K.pyramid_levels(s["ref_img"], 4), K.pyramid_levels(s["cur_img"], 4)
    cur, status, _, border = K.klt_track(rp, cp, px, px, 11, 3, 30, 1e-4, 1e-4)
    assert not border.any()
    t = status == 1
    d = (px[t].astype(np.float32) - cur[t].astype(np.float32)).astype(np.float64)
    disp = np.sort(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    m = len(disp) // 2
    median = float("nan") if len(disp) == 0 else disp[m] if len(disp) % 2 else (disp[m - 1] + disp[m]) / 2.0
    return cur, t, median


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["above", "below"])
def test_gpu_compute_optical_flow_sparse(side):
    ref, cur, px = _frame_pair()
    want_px, tracked, median = _frame_reference(px)
    assert 50 < tracked.sum() < len(px) and 3.0 < median < 6.0  # the shift is (3.3, -2.6): |.| = 4.2
    before = list(ref.features)
    thr = median * (0.999 if side == "above" else 1.001)
    ok = svo_amd.compute_optical_flow_sparse(ref, cur, 11, thr)
    assert ok == (side == "above")
    got = np.array([f.pixel_position for f in cur.features]).reshape(-1, 2)
    assert got.tobytes() == want_px[tracked].tobytes()
    assert all(f.frame is cur and f.level == 0 and f.gradient_magnitude == 0.0 and f.gradient_orientation == 0.0 and
               f.point is None for f in cur.features)
    kept = before if side == "below" else [f for f, t in zip(before, tracked) if t]
    assert len(ref.features) == len(kept) and all(x is y for x, y in zip(ref.features, kept))


@pytest.mark.gpu
def test_gpu_compute_optical_flow_sparse_empty():
    ref, cur, _ = _frame_pair(0)
    assert svo_amd.compute_optical_flow_sparse(ref, cur, 11, 50.0) is True  # NaN median: not below the threshold
    assert len(ref.features) == 0 and len(cur.features) == 0
    # nothing tracked (every point outside the frame): the same NaN path, and the ref features all leave
    ref, cur, _ = _frame_pair(0)
    ref.features = svo_amd.Feature._many(ref, np.array([[-40.2, 10.3], [300.7, 50.1]]))
    assert svo_amd.compute_optical_flow_sparse(ref, cur, 11, 50.0) is True
    assert len(ref.features) == 0 and len(cur.features) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["above", "below", "empty"])
def test_gpu_host_mirror_compute_optical_flow_sparse(side, tmp_path):
    """svo::computeOpticalFlowSparse through `svo_host_check klt`: the feature lists of both frames and the result."""
    s = K.gpu_scene("win11")
    px = s["ref_px"] if side != "empty" else s["ref_px"][:0]
    want_px, tracked, median = _frame_reference(px)
    thr = 50.0 if side == "empty" else median * (0.999 if side == "above" else 1.001)
    np.concatenate([s["ref_img"].ravel(), s["cur_img"].ravel()]).tofile(tmp_path / "images.bin")
    np.ascontiguousarray(px, np.float64).tofile(tmp_path / "px.bin")
    out = subprocess.run([_paths.lib_path("svo_host_check"), "klt", str(tmp_path / "images.bin"), "160", "120",
                          str(tmp_path / "px.bin"), str(len(px)), "11", repr(float(thr))], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    head = lines[0].split()
    assert head[0] == "klt"
    ok, n_ref, n_cur = int(head[1]), int(head[2]), int(head[3])
    assert ok == (0 if side == "below" else 1)

    def rows(tag):
        return np.array([[float.fromhex(v) for v in ln.split()[1:]] for ln in lines if ln.startswith(tag + " ")]).reshape(-1, 2)
    ref_rows, cur_rows = rows("ref"), rows("cur")
    assert len(ref_rows) == n_ref and len(cur_rows) == n_cur
    assert cur_rows.tobytes() == want_px[tracked].tobytes()
    want_ref = px if side == "below" else px[tracked]
    assert ref_rows.tobytes() == np.ascontiguousarray(want_ref).tobytes()
