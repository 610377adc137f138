"""Windowed bundle adjustment (svo_bundle_adjust; BundleAdjustment.two_view_ba / local_ba) against two CPU checkers.

The cost function and the Levenberg-Marquardt schedule are THIS PROJECT'S CONTRACT (include/svo_c.h), modelled on
g2o's OptimizationAlgorithmLevenberg with EdgeProjectXYZ2UV edges, and NOT pinned to g2o: g2o is not part of the
reference tree, so nothing here was compared with its bits.  The checkers are tests/bundle_adjust_ref.py, a numpy
restatement of the contract (float64 or longdouble), and scipy.optimize.least_squares as an independent minimiser
of the same cost.

Tolerances.  T, per output kind, is the largest difference over the committed scenes (bundle_adjust_ref.SCENES)
between the float64 restatement and (a) the same restatement in longdouble, (b) the float64 restatement with the
observation order reversed; the accept / reject sequences of all three are identical.  Measured (x86-64, 80-bit
longdouble):
    rotation matrix entries   2.5e-10      translation           1.5e-08
    points, relative to |X|   1.4e-08      obs_chi2, relative    9.8e-07      init / final chi, relative  4.1e-08
The largest values come from the gauge-free scene loc3 (three free frames, nothing fixed: only the damping
regularises seven directions); the two-view scenes and the 16-frame scene with 4 fixed frames measure 1e-15 to 1e-12
in the poses and 1e-13 to 1e-12 in the points.  The relative obs_chi2 and chi figures are set by tv1, whose exact fit
leaves e2 ~ 1e-11.  test_tolerance_constants re-measures them.  The GPU bound is 8 * T, the rule of C_POINT in
tests/test_two_view_init.py.

scipy.  With max_iterations raised until the restatement's cost stalls (relative decrease below 1e-9), its final
chi against 2 * cost of least_squares(loss='huber', f_scale=delta) over SCIPY_SCENES, one residual sqrt(e2) per edge.
(a) From the same start, 100 evaluations: scipy ends ABOVE the restatement on every scene (excess
chi / chi_scipy - 1 measured: tv63 -0.543, tv65 -0.321, loc3 -0.458, struct -0.096; 3000 evaluations on tv63 still
leave it far above).  One residual |e| per two-dimensional edge gives scipy a Gauss-Newton model of rank
one per edge, so it converges slowly; the largest excess seen is negative and the test asserts excess <= 0: the
restatement is never worse.  (b) So that scipy also says something about the minimum itself, it is started again
from the restatement's stalled estimate (30 evaluations): the largest excess measured is 3.09e-06 (tv65, whose
Huber-weighted tail converges slowly; the others 0 to 5e-14), and the test allows twice that."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import bundle_adjust_ref as B
from common import KITTI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "svo_host_check")

T_ROT, T_TRANS, T_POINT, T_CHI2, T_CHI = 2.5e-10, 1.5e-08, 1.4e-08, 9.8e-07, 4.1e-08
C_GPU = 8.0
SCIPY_SCENES = ("tv63", "tv65", "loc3", "struct")
SCIPY_EXCESS = 0.0          # (a) the largest chi / chi_scipy - 1 measured from the same start is negative
SCIPY_POLISH_EXCESS = 3.09e-06  # (b) the largest measured when scipy starts from the stalled estimate
ALL = list(B.SCENES)
# one batch shares max_iterations and structure_iterations
BATCH = ("loc3", "empty", "loc8", "struct", "loc3r")


def sequence(trace):
    return [(int(t[0]), int(t[1]), int(t[2])) for t in trace]


def differences(a, b):
    """The five kinds of difference between two results (dicts of the restatement's layout), in longdouble."""
    ld = np.longdouble
    pa, pb = np.asarray(a["poses"], ld), np.asarray(b["poses"], ld)
    Xa, Xb = np.asarray(a["points"], ld), np.asarray(b["points"], ld)
    ca, cb = np.asarray(a["obs_chi2"], ld), np.asarray(b["obs_chi2"], ld)
    d = dict(rot=0.0, trans=0.0, point=0.0, chi2=0.0, chi=0.0)
    if len(pa):
        d["rot"] = float(np.abs(B.rotmat(pa[:, :4]) - B.rotmat(pb[:, :4])).max())
        d["trans"] = float(np.abs(pa[:, 4:] - pb[:, 4:]).max())
    if len(Xa):
        d["point"] = float((np.sqrt(((Xa - Xb) ** 2).sum(1)) / np.sqrt((Xb ** 2).sum(1))).max())
        d["chi2"] = float((np.abs(ca - cb) / cb).max())
        d["chi"] = float(max(abs(ld(a[k]) - ld(b[k])) / ld(b[k]) if b[k] else abs(ld(a[k])) for k in ("init_chi", "final_chi")))
    return d


# ---------------------------------------------------------------- CPU
def test_library_and_package_export_the_feature():
    """Fails on a tree without the feature: the C entry point and the Python surface."""
    import svo_amd
    from svo_amd import _capi
    lib = ctypes.CDLL(_capi.lib_path())
    assert hasattr(lib, "svo_bundle_adjust")
    assert "svo_bundle_adjust" in _capi.EXPORTED
    assert callable(svo_amd.bundle_adjust_batch)
    for cls, names in ((svo_amd.BundleAdjustment, ("two_view_ba", "local_ba")), (svo_amd.Map, ("remove_feature", "remove_point")),
                       (svo_amd.Point, ("remove_frame", "number_observation")), (svo_amd.Frame, ("remove_feature",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert svo_amd.BA_MAX_FRAMES == 16


def _c_call(s, frame_off=None, of=None, op=None, poses=None, fixed=None):
    """svo_bundle_adjust with a null context: the layout checks run before the context is looked at."""
    from svo_amd import _capi
    from svo_amd._capi import ptr
    import svo_amd
    poses = np.ascontiguousarray(s.poses if poses is None else poses)
    fixed = np.ascontiguousarray(s.fixed if fixed is None else fixed, np.uint8)
    of = np.ascontiguousarray(s.obs_frame if of is None else of, np.int32)
    op = np.ascontiguousarray(s.obs_point if op is None else op, np.int32)
    pts, px = np.ascontiguousarray(s.points), np.ascontiguousarray(s.obs_px)
    fo = np.array([0, len(poses)] if frame_off is None else frame_off, np.int32)
    po, oo = np.array([0, len(pts)], np.int32), np.array([0, len(of)], np.int32)
    chi2, ic, fc = np.zeros(len(of)), np.zeros(1), np.zeros(1)
    it, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cam = svo_amd.PinholeCamera.kitti().as_c()
    L = _capi.lib()
    r = L.svo_bundle_adjust(None, ctypes.byref(cam), 1, ptr(fo), ptr(po), ptr(oo), ptr(poses), ptr(fixed), ptr(pts),
                            ptr(of), ptr(op), ptr(px), 2.0, 10, 0, ptr(chi2), ptr(ic), ptr(fc), ptr(it), ptr(st), None)
    return r, L.svo_last_error().decode()


def bad_layouts():
    s = B.scene("tv2")
    yield "17 frames", dict(poses=np.tile(s.poses[:1], (17, 1)), fixed=np.zeros(17, np.uint8)), "17 frames"
    yield "duplicate", dict(of=[0, 0, 0, 1]), "duplicate"
    yield "ungrouped", dict(op=[0, 1, 0, 1]), "grouped"
    yield "frame index", dict(of=[0, 2, 0, 1]), "frame index"
    s3 = B.Scene(5, 2, 1, 3)
    yield "single observation", dict(scene=s3, of=s3.obs_frame[:5], op=s3.obs_point[:5]), "fewer than two"


def test_layout_errors_are_codes():
    from svo_amd import _capi
    r, msg = _c_call(B.scene("tv2"))
    assert r == _capi.SVO_ERR_ARG and "ctx" in msg  # a good layout reaches the context check
    for name, kw, word in bad_layouts():
        s = kw.pop("scene", B.scene("tv2"))
        r, msg = _c_call(s, **kw)
        assert r == _capi.SVO_ERR_ARG and word in msg, (name, r, msg)


def test_jacobians_against_central_differences():
    """J_p (pose <- exp(dp) * pose) and J_x of the restatement against central differences of proj(T X)."""
    s = B.scene("loc8")
    f, cx, cy = KITTI["fx"], KITTI["cx"], KITTI["cy"]
    of, op = s.obs_frame.astype(int), s.obs_point.astype(int)

    def proj(poses, X):
        c = np.einsum("mij,mj->mi", B.rotmat(poses[:, :4])[of], X[op]) + poses[of, 4:]
        return np.stack([f * c[:, 0] / c[:, 2] + cx, f * c[:, 1] / c[:, 2] + cy], 1), c

    _, c = proj(s.poses, s.points)
    Jp, Jx = B.jacobians(B.rotmat(s.poses[:, :4]), of, c, f)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        plus = np.array([B.se3_compose(B.se3_exp(d), p) for p in s.poses])
        minus = np.array([B.se3_compose(B.se3_exp(-d), p) for p in s.poses])
        num = (proj(plus, s.points)[0] - proj(minus, s.points)[0]) / (2 * h)
        assert np.abs(num - Jp[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(Jp[:, :, k]).max()), k
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        num = (proj(s.poses, s.points + d)[0] - proj(s.poses, s.points - d)[0]) / (2 * h)
        assert np.abs(num - Jx[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(Jx[:, :, k]).max()), k


def test_noise_free_scene_is_recovered():
    """No pixel noise, perturbed start, two fixed frames (they fix the gauge, scale included): chi falls below
    1e-12 * init_chi and the positions come back."""
    s = B.Scene(7, 4, 2, 60, 2, 4, noise=0.0)
    r = s.run(max_iterations=30)
    print("noise-free: init", r["init_chi"], "final", r["final_chi"], "iterations", r["iterations"])
    assert r["final_chi"] < 1e-12 * r["init_chi"]
    rel = np.linalg.norm(r["points"] - s.true_points, axis=1) / np.linalg.norm(s.true_points, axis=1)
    dp = differences(dict(poses=r["poses"], points=[], obs_chi2=[]), dict(poses=s.true_poses, points=[], obs_chi2=[]))
    print("noise-free: point error", rel.max(), "rotation", dp["rot"], "translation", dp["trans"])
    assert rel.max() < 1e-6 and dp["rot"] < 1e-7 and dp["trans"] < 1e-6


@functools.lru_cache(maxsize=None)
def stalled(name):
    """The restatement run until its cost stalls: max_iterations doubled until an accepted step lowers chi by less
    than 1e-9 relative (or the problem terminates)."""
    s = B.scene(name)
    n = 10
    while True:
        r = s.run(max_iterations=n)
        chis = [float(r["init_chi"])] + [float(t[5]) for t in r["trace"] if t[2]]
        dec = [(a - b) / a for a, b in zip(chis, chis[1:])]
        if r["status"] == 1 or (dec and dec[-1] < 1e-9) or n >= 640:
            return r, n
        n *= 2


def scipy_minimum(s, poses0, points0, max_nfev):
    """2 * cost of least_squares on one residual sqrt(e2) per edge with loss='huber', f_scale=delta, from poses0 /
    points0.  The Jacobian is central differences, taken in groups: the points are independent of each other."""
    from scipy.optimize import least_squares
    free = np.nonzero(s.fixed == 0)[0]
    nf = len(free)
    of, op = s.obs_frame.astype(int), s.obs_point.astype(int)
    f, cx, cy = KITTI["fx"], KITTI["cx"], KITTI["cy"]

    def residual(x):
        poses = poses0.copy()
        for k, i in enumerate(free):
            poses[i] = B.se3_compose(B.se3_exp(x[6 * k:6 * k + 6]), poses0[i])
        X = points0 + x[6 * nf:].reshape(-1, 3)
        return np.sqrt(B.edges(B.rotmat(poses[:, :4]), poses[:, 4:], X, of, op, s.obs_px, f, cx, cy, s.delta)[2])

    def jac(x):
        M, h = len(of), 1e-6
        J = np.zeros((M, len(x)))
        for k in range(6 * nf):
            d = np.zeros_like(x)
            d[k] = h
            J[:, k] = (residual(x + d) - residual(x - d)) / (2 * h)
        for k in range(3):
            d = np.zeros_like(x)
            d[6 * nf + k::3] = h
            J[np.arange(M), 6 * nf + 3 * op + k] = (residual(x + d) - residual(x - d)) / (2 * h)
        return J

    sol = least_squares(residual, np.zeros(6 * nf + 3 * len(points0)), jac=jac, loss="huber", f_scale=s.delta,
                        x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-12, max_nfev=max_nfev)
    return 2.0 * sol.cost


def test_stalled_cost_against_scipy():
    """Costs, never parameters: the gauge is free.  See the module docstring for the two comparisons."""
    worst, worst_polish = -np.inf, -np.inf
    for name in SCIPY_SCENES:
        s = B.scene(name)
        r, n = stalled(name)
        chi = float(r["final_chi"])
        same_start = scipy_minimum(s, s.poses, s.points, 100)
        polished = scipy_minimum(s, np.asarray(r["poses"]), np.asarray(r["points"]), 30)
        print(f"scipy {name}: restatement {chi:.12g} after max_iterations {n}; scipy from the same start "
              f"{same_start:.12g}, excess {chi / same_start - 1:.3g}; from the stalled estimate {polished:.12g}, "
              f"excess {chi / polished - 1:.3g}")
        worst = max(worst, chi / same_start - 1)
        worst_polish = max(worst_polish, chi / polished - 1)
    assert worst <= 2 * SCIPY_EXCESS
    assert worst_polish <= 2 * SCIPY_POLISH_EXCESS


def test_tolerance_constants():
    """Re-measures T (module docstring): float64 against longdouble and against the reversed observation order, with
    identical accept / reject sequences."""
    worst = dict(rot=0.0, trans=0.0, point=0.0, chi2=0.0, chi=0.0)
    for name in ALL:
        a = B.reference(name)
        for other in (B.reference(name, "longdouble"), B.reference(name, "float64", True)):
            assert sequence(a["trace"]) == sequence(other["trace"]), name
            assert a["iterations"] == other["iterations"] and a["status"] == other["status"]
            for k, v in differences(a, other).items():
                worst[k] = max(worst[k], v)
    print("measured T:", worst)
    assert worst["rot"] <= T_ROT and worst["trans"] <= T_TRANS and worst["point"] <= T_POINT
    assert worst["chi2"] <= T_CHI2 and worst["chi"] <= T_CHI
    # the constants are the measurement, not a generous cover of it
    assert worst["rot"] >= T_ROT / 2 and worst["trans"] >= T_TRANS / 2 and worst["point"] >= T_POINT / 2


def test_scene_conditions():
    """What makes the exact comparisons of the GPU tests complete: no borderline accept / reject decision, no edge
    at the removal threshold, a rejected trial and gross outliers among the scenes."""
    rejected, over = 0, 0
    for name in ALL:
        s, r = B.scene(name), B.reference(name)
        assert r["trace"], name
        assert min(abs(float(t[4])) for t in r["trace"]) >= 1e-3, name
        thr = s.delta * s.delta
        assert np.abs(r["obs_chi2"] / thr - 1.0).min() >= 1e-6, name
        rejected += sum(1 for t in r["trace"] if not t[2])
        over += int((r["obs_chi2"] > thr).sum())
    assert B.reference("loc3r")["status"] == 0 and sum(1 for t in B.reference("loc3r")["trace"] if not t[2]) >= 1
    assert rejected >= 1 and over >= 1
    s = B.scene("loc16")
    assert len(s.poses) == 16 and int(s.fixed.sum()) == 4 and len(s.points) == 120
    n_obs = np.bincount(s.obs_point)
    assert n_obs.min() >= 2 and n_obs.max() <= 16


# ---------------------------------------------------------------- GPU
class Empty:
    """Two frames and nothing else: status -1, poses as given."""
    cam, delta = KITTI, 2.0
    poses = B.Scene(1, 2, 1, 1).poses
    fixed = np.array([1, 0], np.uint8)
    points, obs_px = np.zeros((0, 3)), np.zeros((0, 2))
    obs_frame = obs_point = np.zeros(0, np.int32)


def get_scene(name):
    return Empty if name == "empty" else B.scene(name)


def run_gpu(names, max_iterations, structure_iterations, camera=None):
    """One svo_bundle_adjust call over the named scenes; per scene a dict of the restatement's layout."""
    import svo_amd
    camera = camera or svo_amd.PinholeCamera.kitti()
    ss = [get_scene(n) for n in names]
    off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    fo, po, oo = off([len(s.poses) for s in ss]), off([len(s.points) for s in ss]), off([len(s.obs_frame) for s in ss])
    poses = np.ascontiguousarray(np.concatenate([s.poses for s in ss]))
    points = np.ascontiguousarray(np.concatenate([s.points for s in ss]))
    r = svo_amd.bundle_adjust_batch(camera, fo, po, oo, poses, np.concatenate([s.fixed for s in ss]),
                                    points, np.concatenate([s.obs_frame for s in ss]),
                                    np.concatenate([s.obs_point for s in ss]), np.concatenate([s.obs_px for s in ss]),
                                    2.0, max_iterations, structure_iterations, trace=True)
    out = {}
    for k, n in enumerate(names):
        tr = r.trace[k]
        out[n] = dict(poses=poses[fo[k]:fo[k + 1]], points=points[po[k]:po[k + 1]], obs_chi2=r.obs_chi2[oo[k]:oo[k + 1]],
                      init_chi=r.init_chi[k], final_chi=r.final_chi[k], iterations=int(r.iterations[k]),
                      status=int(r.status[k]), trace=[tuple(t) for t in tr[tr[:, 0] >= 0]])
    raw = b"".join(np.ascontiguousarray(a).tobytes() for a in (poses, points, r.obs_chi2, r.init_chi, r.final_chi,
                                                               r.iterations, r.status, r.trace))
    return out, raw


@functools.lru_cache(maxsize=None)
def gpu_single(name):
    s = B.scene(name)
    return run_gpu((name,), s.max_iterations, s.structure_iterations)


def check_against_restatement(name, got):
    s, want = B.scene(name), B.reference(name)
    print(name, "GPU trace", [(int(t[0]), int(t[1]), int(t[2]), float(t[3]), float(t[4])) for t in got["trace"]])
    assert sequence(got["trace"]) == sequence(want["trace"])
    assert got["iterations"] == want["iterations"] and got["status"] == want["status"]
    d = differences(got, want)
    print(name, "GPU - restatement:", d)
    assert d["rot"] <= C_GPU * T_ROT and d["trans"] <= C_GPU * T_TRANS and d["point"] <= C_GPU * T_POINT
    assert d["chi2"] <= C_GPU * T_CHI2 and d["chi"] <= C_GPU * T_CHI
    thr = s.delta * s.delta
    assert np.array_equal(got["obs_chi2"] > thr, want["obs_chi2"] > thr)
    fixed = s.fixed.astype(bool)
    assert np.array_equal(got["poses"][fixed], s.poses[fixed])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_gpu_against_restatement(name):
    """Accept / reject sequence, iterations and status exact; poses, points, obs_chi2 and the sums within 8 * T; the
    over-threshold flags exact; a second call returns the same bytes."""
    got, raw = gpu_single(name)
    check_against_restatement(name, got[name])
    s = B.scene(name)
    again = run_gpu((name,), s.max_iterations, s.structure_iterations)[1]
    assert again == raw


@pytest.mark.gpu
def test_gpu_batch_of_unequal_problems():
    """Five unequal problems in one call, one of them without points: each equals its own single-problem call to the
    bit, the empty one reports status -1 and keeps its poses."""
    got, _ = run_gpu(BATCH, 10, 10)
    e = got["empty"]
    assert e["status"] == -1 and e["iterations"] == 0 and e["init_chi"] == 0.0 and e["final_chi"] == 0.0
    assert np.array_equal(e["poses"], Empty.poses) and not e["trace"]
    for name in BATCH:
        if name == "empty":
            continue
        check_against_restatement(name, got[name])
        single = gpu_single(name)[0][name]
        for k in ("poses", "points", "obs_chi2"):
            assert np.array_equal(got[name][k], single[k]), (name, k)
        assert got[name]["trace"] == single["trace"]


@pytest.mark.gpu
def test_gpu_fx_on_both_axes():
    """Quirk kept: setupG2o passes g2o::CameraParameters(fx, principalPoint, 0) (src/bundle_adjustment.cpp:333), so
    fy never reaches the cost.  A camera with another fy returns the same bytes."""
    import svo_amd
    k = svo_amd.PinholeCamera.kitti()
    other = svo_amd.PinholeCamera(k.width, k.height, k.fx, 0.5 * k.fy, k.cx, k.cy)
    assert run_gpu(("tv63",), 10, 0, other)[1] == gpu_single("tv63")[1]


@pytest.mark.gpu
def test_gpu_argument_errors():
    import svo_amd
    cam = svo_amd.PinholeCamera.kitti()
    for name, kw, word in bad_layouts():
        s = kw.pop("scene", B.scene("tv2"))
        poses = np.ascontiguousarray(kw.get("poses", s.poses)).copy()
        pts = np.ascontiguousarray(s.points).copy()
        of, op = kw.get("of", s.obs_frame), kw.get("op", s.obs_point)
        with pytest.raises(svo_amd.SvoError) as e:
            svo_amd.bundle_adjust_batch(cam, [0, len(poses)], [0, len(pts)], [0, len(of)], poses, kw.get("fixed", s.fixed),
                                        pts, of, op, s.obs_px[:len(of)], 2.0)
        assert word in str(e.value), (name, str(e.value))
        assert np.array_equal(poses, kw.get("poses", s.poses)) and np.array_equal(pts, s.points)


# ---------------------------------------------------------------- objects
def numpy_removal(edges, chi2, thr, n_points):
    """Map::removeFeature over the edges whose e2 exceeds thr, in edge order, on plain lists: returns the set of
    surviving edge indices and the deleted points.  edges: (frame, point) per edge."""
    obs = {j: [k for k, e in enumerate(edges) if e[1] == j] for j in range(n_points)}
    alive = set(range(len(edges)))
    deleted = set()
    has_point = [True] * len(edges)
    for k in np.nonzero(chi2 > thr)[0]:
        j = edges[k][1]
        if not has_point[k]:
            continue
        if len(obs[j]) <= 2:
            alive -= set(obs[j])
            obs[j] = []
            deleted.add(j)
            has_point[k] = False
            continue
        obs[j] = [q for q in obs[j] if edges[q][0] != edges[k][0]]
        alive.discard(k)
    return alive, deleted


def build_graph(poses, points, edges, px):
    """Frames, Points and one Feature per edge, appended to its frame and its point in edge order."""
    import svo_amd
    cam = svo_amd.PinholeCamera.kitti()
    img = np.zeros((cam.height, cam.width), np.uint8)
    frames = []
    for p in poses:
        fr = svo_amd.Frame(cam, img, 1)
        fr.abs_pose = np.array(p, np.float64)
        frames.append(fr)
    pts = [svo_amd.Point(x) for x in points]
    feats = []
    for (i, j), u in zip(edges, px):
        f = svo_amd.Feature(frames[i], u, point=pts[j])
        frames[i].add_feature(f)
        pts[j].add_feature(f)
        feats.append(f)
    return cam, frames, pts, feats


def check_graph(frames, pts, feats, edges, alive, deleted):
    import svo_amd
    for i, fr in enumerate(frames):
        want = [feats[k] for k in sorted(alive) if edges[k][0] == i]
        assert len(fr.features) == len(want) and all(a is b for a, b in zip(fr.features, want)), i
        px, _, pos, has = fr.feature_arrays()  # coherent with the objects after the removals
        assert np.array_equal(px, np.array([f.pixel_position for f in want]).reshape(-1, 2))
        assert np.array_equal(pos, np.array([f.point.position for f in want]).reshape(-1, 3)) and has.all()
    for j, p in enumerate(pts):
        if j in deleted:
            assert p.type == svo_amd.PointType.DELETED and p.number_observation() == 0
            assert not any(f.point is p for fr in frames for f in fr.features)
        else:
            assert p.type != svo_amd.PointType.DELETED
            assert [f for f in p.features] == [feats[k] for k in sorted(alive) if edges[k][1] == j]


@pytest.mark.gpu
def test_gpu_two_view_ba_after_initialize():
    """two_view_ba on the frames two_view_initialize leaves: poses and positions as the restatement's on the same
    arrays (8 * T), the removed features as Map::removeFeature on plain lists gives them."""
    import svo_amd
    import two_view_ref as TV
    s = TV.make_scene(seed=105, n=130)
    cam = svo_amd.PinholeCamera.kitti()
    img = np.zeros((cam.height, cam.width), np.uint8)
    ref, cur = svo_amd.Frame(cam, img, 1), svo_amd.Frame(cam, img, 1)
    ref.abs_pose[:] = s.ref_pose
    ref.features = svo_amd.Feature._many(ref, s.ref_px)
    cur.features = svo_amd.Feature._many(cur, s.cur_px)
    ok, _, n = svo_amd.two_view_initialize(ref, cur, s.E, 2.0, 30)
    assert ok and n > 50
    rng = np.random.default_rng(3)
    for k in rng.choice(n, 6, replace=False):  # gross mismatches for the removal to find
        cur.features[k].pixel_position = cur.features[k].pixel_position + np.array([9.0, -7.0])
    poses = np.array([ref.abs_pose, cur.abs_pose])
    points = np.array([f.point.position for f in ref.features])
    edges = [(i, j) for j in range(n) for i in (0, 1)]
    px = np.array([fr.features[j].pixel_position for j in range(n) for fr in (ref, cur)])
    want = B.bundle_adjust(KITTI, poses, [1, 0], points, [e[0] for e in edges], [e[1] for e in edges], px, 2.0, 10, 0)
    assert min(abs(float(t[4])) for t in want["trace"]) >= 1e-3
    assert np.abs(want["obs_chi2"] / 4.0 - 1.0).min() >= 1e-6
    feats = [fr.features[j] for j in range(n) for fr in (ref, cur)]
    pts = [f.point for f in ref.features]
    m = svo_amd.Map(cam, 30)
    ba = svo_amd.BundleAdjustment(cam)
    init_chi, final_chi, removed = ba.two_view_ba(ref, cur, m, 2.0)
    got = dict(poses=np.array([ref.abs_pose, cur.abs_pose]), points=np.array([p.position for p in pts]),
               obs_chi2=want["obs_chi2"], init_chi=init_chi, final_chi=final_chi)
    d = differences(got, want)
    print("two_view_ba - restatement:", d, "removed", removed)
    assert d["rot"] <= C_GPU * T_ROT and d["trans"] <= C_GPU * T_TRANS and d["point"] <= C_GPU * T_POINT and d["chi"] <= C_GPU * T_CHI
    assert np.array_equal(ref.abs_pose, s.ref_pose)
    assert removed == int((want["obs_chi2"] > 4.0).sum()) and removed >= 6
    alive, deleted = numpy_removal(edges, want["obs_chi2"], 4.0, n)
    assert deleted and len(alive) == 2 * (n - len(deleted))
    check_graph([ref, cur], pts, feats, edges, alive, deleted)


def four_keyframe_case():
    """Four keyframes and one older frame outside the list; 50 points with 2 to 5 observations, 5 % gross
    outliers.  Edges are listed frame by frame, so the points' first-seen order is not their index order."""
    s = B.Scene(11, 5, 1, 50, 2, 5, outliers=0.05)
    order = np.lexsort((s.obs_point, (s.obs_frame + 4) % 5))  # frames 1 2 3 4 (the keyframes), then frame 0
    frame_of = (s.obs_frame[order] + 4) % 5                  # keyframes 0..3, the outside frame 4
    poses = np.concatenate([s.poses[1:], s.poses[:1]])
    return s, poses, [(int(i), int(j)) for i, j in zip(frame_of, s.obs_point[order])], s.obs_px[order]


def first_seen_problem(edges, n_key):
    """local_ba's problem from the edge list: points in first-seen order over the keyframes, edges grouped by point
    in each point's own observation order."""
    seen = []
    for i in range(n_key):
        for k, e in enumerate(edges):
            if e[0] == i and e[1] not in seen:
                seen.append(e[1])
    ks = [k for j in seen for k, e in enumerate(edges) if e[1] == j]
    return seen, ks


@pytest.mark.gpu
def test_gpu_local_ba_on_a_four_keyframe_map(tmp_path):
    import svo_amd
    s, poses, edges, px = four_keyframe_case()
    cam, frames, pts, feats = build_graph(poses, s.points, edges, px)
    m = svo_amd.Map(cam, 30)
    m.key_frames = frames[:4]
    seen, ks = first_seen_problem(edges, 4)
    assert len(seen) == len(pts)  # every point has two observations or more and a keyframe among them
    rank = {j: r for r, j in enumerate(seen)}
    want = B.bundle_adjust(KITTI, poses, [0, 0, 0, 0, 1], s.points[seen], [edges[k][0] for k in ks],
                           [rank[edges[k][1]] for k in ks], px[ks], 2.0, 10, 10)
    assert min(abs(float(t[4])) for t in want["trace"]) >= 1e-3
    assert np.abs(want["obs_chi2"] / 4.0 - 1.0).min() >= 1e-6
    ba = svo_amd.BundleAdjustment(cam)
    init_chi, final_chi, removed = ba.local_ba(m, 2.0)
    got_points = np.array([pts[j].position for j in seen])
    got = dict(poses=np.array([fr.abs_pose for fr in frames]), points=got_points, obs_chi2=want["obs_chi2"],
               init_chi=init_chi, final_chi=final_chi)
    d = differences(got, want)
    print("local_ba - restatement:", d, "removed", removed)
    assert d["rot"] <= C_GPU * T_ROT and d["trans"] <= C_GPU * T_TRANS and d["point"] <= C_GPU * T_POINT and d["chi"] <= C_GPU * T_CHI
    assert np.array_equal(frames[4].abs_pose, poses[4])  # the frame outside the keyframe list is fixed
    assert removed == int((want["obs_chi2"] > 4.0).sum()) and removed >= 1
    chi2 = np.zeros(len(edges))
    chi2[ks] = want["obs_chi2"]
    # removal runs in the problem's edge order (ks), not the construction order
    alive_r, deleted_r = numpy_removal([(edges[k][0], rank[edges[k][1]]) for k in ks], want["obs_chi2"], 4.0, len(seen))
    alive = {ks[q] for q in alive_r}
    deleted = {seen[r] for r in deleted_r}
    check_graph(frames, pts, feats, edges, alive, deleted)
    big = svo_amd.Map(cam, 30)  # 17 frames in one problem
    big.key_frames = [svo_amd.Frame(cam, np.zeros((cam.height, cam.width), np.uint8), 1) for _ in range(17)]
    with pytest.raises(ValueError, match="17 frames"):
        ba.local_ba(big, 2.0)
    # the C++ mirror on the same graph: the same library call, so the same bits
    path = os.path.join(str(tmp_path), "wba.bin")
    np.concatenate([[KITTI[k] for k in ("fx", "fy", "cx", "cy", "width", "height")], [2.0, 1, 4, 5], poses.ravel(),
                    [len(s.points)], s.points.ravel(), [len(edges)],
                    np.concatenate([np.array(edges, np.float64), px], axis=1).ravel()]).astype(np.float64).tofile(path)
    out = subprocess.run([HOST_CHECK, "wba", path], capture_output=True, text=True, timeout=60, check=True).stdout
    lines = [ln.split() for ln in out.strip().split("\n")]
    assert lines[0][0] == "chi" and [float.fromhex(x) for x in lines[0][1:3]] == [init_chi, final_chi]
    assert int(lines[0][3]) == removed
    got_pose = np.array([[float.fromhex(x) for x in ln[1:]] for ln in lines if ln[0] == "pose"])
    assert np.array_equal(got_pose, np.array([fr.abs_pose for fr in frames]))
    assert [int(ln[1]) for ln in lines if ln[0] == "left"] == [len(fr.features) for fr in frames]
    rows = [ln for ln in lines if ln[0] == "pt"]
    assert np.array_equal(np.array([[float.fromhex(x) for x in ln[1:4]] for ln in rows]), np.array([p.position for p in pts]))
    assert [(int(ln[4]), int(ln[5])) for ln in rows] == [(p.type, p.number_observation()) for p in pts]
