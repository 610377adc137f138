"""Two-view map initialisation (System::processSecondFrame from the essential matrix on, src/system.cpp:144-223):
svo_two_view_init / svo_triangulate_dlt (csrc/two_view.hip), svo_amd.two_view_init_batch / triangulate_batch /
two_view_initialize and the C++ mirror (host/svo.hpp initializeTwoView via build/svo_host_check init).

The checker is the numpy float64 restatement of tests/two_view_ref.py (numpy.linalg.svd, matrix-form poses, its own
3x3 elimination).  Eigen and OpenCV are absent, so parity with the reference binary itself is not pinned here.

What is compared, and how tightly:
  F                  |dF| <= 1e-14 * (|invK^T| |E| |invK|) entry by entry (two 3x3 products);
  Sampson pixels     bit-exact against the restatement evaluated with the F the call returned (the same IEEE
                     operations in the same order, no contraction);
  counts / winner / valid / survivor / n_valid   exact.  A match could be left out only if its decision were
                     borderline in the restatement (|z| < 1e-9 |X| in a camera, a corrected pixel within 1e-9 px of
                     an isInFrame threshold); the committed seeds have no such match (asserted on the CPU);
  the four hypotheses   as a set: which rotation an SVD calls R1 and which sign it gives t is a convention (Eigen's
                     cannot be consulted, numpy's differs from the product's Jacobi SVD), so the call's labelling is
                     matched to numpy's through one of the four relabelings t <-> -t, R1 <-> R2 that reproduces the
                     counts, and the winner must be the first strictly largest count in the call's own order;
  winning cur_pose   rotation matrix and translation within 1e-12 of the restatement;
  points             per match |X - X_np| / |X_np| <= C_POINT * eps * cond(A^T A), cond of that match's 3x3 normal
                     matrix.  C_POINT = 8 * C_RATIO, where C_RATIO is the largest rel_err / (eps * cond) between the
                     float64 restatement and the same restatement in numpy.longdouble over every committed scene
                     (test_point_tolerance_constant measures it: 7.949, on side2000 -> C_RATIO = 8.0, C_POINT = 64);
  median_depth       bit-equal to algorithm::computeMedian of the depth vector the call returned: numpy's order
                     statistic for odd counts, tests/cpp/median_check.cpp (the real std::nth_element) for even ones.
Scenes: the KITTI camera, reference pixels uniform >= 20 px inside the frame, depths 6-60, a small rotation plus a
sideways-dominant translation (one scene: forward motion, matches near the epipole), current pixels = projection +
N(0, 0.3 px).  Counts 1, 2, 63, 64, 65, 257, 2000 as single pairs and one batch of three unequal pairs (a non-identity
reference pose, a pair without matches that fails, forward motion).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import two_view_ref as TV
from common import KITTI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "svo_host_check")
EPS = TV.EPS
MAP_SCALE, CELL = 2.0, 30
C_RATIO = 8.0
C_POINT = 8 * C_RATIO
POSED = TV.Rt_to_pose(TV.rodrigues(np.array([0.004, -0.007, 0.003])), np.array([0.05, -0.02, 0.08]))

# name -> make_scene arguments (+ map_scale)
SCENES = {
    "side1": dict(seed=101, n=1), "side2": dict(seed=102, n=2), "side63": dict(seed=103, n=63),
    "side64": dict(seed=104, n=64), "side65": dict(seed=105, n=65), "side257": dict(seed=106, n=257),
    "side2000": dict(seed=107, n=2000),
    "posed130": dict(seed=108, n=130, ref_pose=POSED),
    "empty": dict(seed=109, n=0),
    "forward257": dict(seed=110, n=257, kind="forward"),
    "exact257": dict(seed=111, n=257, noise=0.0, map_scale=1.0),
}
BATCHES = [[k] for k in ("side1", "side2", "side63", "side64", "side65", "side257", "side2000", "exact257")] + \
          [["posed130", "empty", "forward257"]]
IN_BATCHES = [k for b in BATCHES for k in b]


@functools.lru_cache(maxsize=None)
def scene(name):
    kw = dict(SCENES[name])
    ms = kw.pop("map_scale", MAP_SCALE)
    s = TV.make_scene(**kw)
    s.map_scale = ms
    return s


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("two_view")


_restated = {}


def restated(name, tmp, F=None, dtype=np.float64):
    key = (name, None if F is None else F.tobytes(), dtype)
    if key not in _restated:
        s = scene(name)
        _restated[key] = TV.two_view_init(s.E, s.ref_pose, s.ref_px, s.cur_px, s.map_scale, CELL, tmp, F=F, dtype=dtype)
    return _restated[key]


def first_strict_max(counts):
    w, best = -1, 0
    for h in range(4):
        if counts[h] > best:
            best, w = int(counts[h]), h
    return w


def check_pair(name, got, tmp):
    """One pair's outputs `got` (attributes as svo_amd.TwoViewResult, plus ref_px / cur_px) against the
    restatement.  Returns the largest points ratio rel_err / (eps * cond) it saw."""
    s = scene(name)
    n = s.n
    own = restated(name, tmp)
    assert np.all(np.abs(got.F - own.F) <= 1e-14 * TV.fundamental_bound(s.E)), np.abs(got.F - own.F).max()
    ref = restated(name, tmp, F=np.ascontiguousarray(got.F))
    assert np.array_equal(got.ref_px, ref.ref_px) and np.array_equal(got.cur_px, ref.cur_px)
    assert not ref.borderline.any()  # nothing is left out of the exact comparisons
    perms = [p for p in TV.RELABELINGS if all(ref.counts[p[h]] == got.counts[h] for h in range(4))]
    assert perms, (got.counts, ref.counts)
    assert got.winner == first_strict_max(got.counts)
    if n == 0 or ref.winner < 0:
        assert got.winner == -1 and not got.counts.any() and got.n_valid == 0 and np.isnan(got.median_depth)
        assert np.isnan(got.cur_pose).all()  # the caller's row (NaN in the Python mirror) is left alone
        assert not got.valid.any() and np.all(got.survivor == -1)
        return 0.0
    assert ref.unique_winner
    assert any(p[got.winner] == ref.winner for p in perms), (got.winner, ref.winner, perms)
    Rg, tg = TV.pose_to_Rt(got.cur_pose)
    assert np.abs(Rg - ref.cur_R).max() <= 1e-12 and np.abs(tg - ref.cur_t).max() <= 1e-12
    assert np.array_equal(got.valid, ref.valid) and got.n_valid == ref.n_valid
    assert np.array_equal(got.survivor, ref.survivor)
    rel = np.linalg.norm(got.points_world - ref.points_world, axis=1) / np.linalg.norm(ref.points_world, axis=1)
    ratio = rel / (EPS * ref.cond)
    print(f"{name}: counts {got.counts.tolist()} winner {got.winner} valid {got.n_valid}/{n} "
          f"cond max {ref.cond.max():.3g} points ratio max {ratio.max():.4g} (bound {C_POINT})")
    assert np.all(ratio <= C_POINT), (ratio.max(), int(ratio.argmax()))
    assert got.median_depth == TV.reference_median(got.depth, tmp)[2]
    return float(ratio.max())


# ------------------------------------------------------------------ CPU: the restatement itself
@pytest.mark.parametrize("name", ["exact257"])
def test_restatement_recovers_true_motion(name, tmp):
    s, r = scene(name), restated(name, tmp)
    assert sorted(r.counts.tolist()) == [0, 0, 0, s.n] and r.unique_winner
    Rw, tw = r.hyp[r.winner]
    assert np.abs(Rw - s.R_true).max() <= 1e-12
    assert np.abs(tw - s.t_true / np.linalg.norm(s.t_true)).max() <= 1e-12  # up to scale: a unit translation
    # the points sit on their reference rays at one common multiple of the true depth (identity reference pose)
    v = np.nonzero(r.valid)[0]
    ratio = r.points_world[v, 2] / s.depth_true[v]
    assert np.abs(ratio / ratio[0] - 1).max() <= C_POINT * EPS * r.cond.max()
    assert abs(np.median(np.linalg.norm(r.points_cur_scaled, axis=1)) / s.map_scale - 1) <= C_POINT * EPS * r.cond.max()


@pytest.mark.parametrize("name", IN_BATCHES)
def test_no_borderline_decisions(name, tmp):
    """The cap on matches left out of the exact comparisons is zero: no committed scene has a borderline one, and
    the vote has one winner by a wide margin."""
    s, r = scene(name), restated(name, tmp)
    assert not r.borderline.any()
    if s.n:
        assert r.winner >= 0 and r.unique_winner
        assert sorted(r.counts.tolist())[2] * 10 <= r.counts.max() or s.n < 10
        assert 0.85 * s.n <= r.n_valid or s.n < 10  # most matches make a point
    else:
        assert r.winner == -1


def test_point_tolerance_constant(tmp):
    """C_RATIO is the largest rel_err / (eps * cond(A^T A)) between the float64 restatement and the same
    restatement in numpy.longdouble over every committed scene, rounded up; C_POINT is 8 times it.  Measured
    (cond max / ratio max): side64 1.6e5 / 0.66, side65 1.3e5 / 0.89, side257 2.1e5 / 3.2, side2000 2.2e5 / 7.949,
    exact257 1.7e5 / 2.1, posed130 3.9e7 / 2.0, forward257 1.4e10 / 3.1 -> C_RATIO = 8.0."""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("numpy.longdouble is not wider than float64 on this platform")
    worst = 0.0
    for name in IN_BATCHES:
        if scene(name).n == 0:
            continue
        a, b = restated(name, tmp), restated(name, tmp, dtype=np.longdouble)
        assert a.winner == b.winner and a.median_index == b.median_index
        d = (a.points_world.astype(np.longdouble) - b.points_world)
        rel = np.sqrt((d * d).sum(axis=1)) / np.sqrt((b.points_world ** 2).sum(axis=1))
        ratio = (rel / (EPS * a.cond)).astype(np.float64)
        print(f"{name}: cond max {a.cond.max():.3g} ratio max {ratio.max():.4g}")
        worst = max(worst, float(ratio.max()))
    print("largest ratio", worst)
    assert worst <= C_RATIO <= 1.25 * worst + 0.005, worst


def test_median_tool_matches_order_statistics(tmp):
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 64, 65, 2000):
        v = rng.uniform(1.0, 50.0, n)
        lo, hi, med = TV.reference_median(v, tmp)
        srt = np.sort(v)
        assert hi == srt[n // 2] and med == (lo + hi) / 2.0
        assert lo in v and lo <= hi  # vec[mid-1]: some element below the pivot, not always the next order statistic


def test_abi_argument_validation():
    """Both calls reject bad sizes and null pointers with SVO_ERR_ARG and a message, before any device is needed."""
    from svo_amd import _capi
    L = _capi.lib()
    cam = _capi.SvoCamera(KITTI["fx"], KITTI["fy"], KITTI["cx"], KITTI["cy"], KITTI["width"], KITTI["height"])
    off = np.array([0, 2], np.int32)
    bad = np.array([0, 3, 2], np.int32)
    d = np.zeros(64)
    i4 = np.zeros(8, np.int32)
    u1 = np.zeros(8, np.uint8)
    P = _capi.ptr

    def init(ctx=None, n_pairs=1, feat_off=off, scale=1.0, cell=30, E=d):
        return L.svo_two_view_init(ctx, ctypes.byref(cam), n_pairs, P(feat_off), P(E), P(d), scale, cell, P(d), P(d),
                                   P(d), P(i4), P(i4), P(d), P(d), P(i4), P(d), P(u1), P(i4), P(d))

    def tri(ctx=None, n_pairs=1, feat_off=off, px=d):
        return L.svo_triangulate_dlt(ctx, ctypes.byref(cam), n_pairs, P(feat_off), P(d), P(d), P(px), P(d), P(d))

    for call, kw, text in ((init, {}, b"null"), (init, dict(n_pairs=-1), b"n_pairs"), (init, dict(feat_off=None), b"null"),
                           (init, dict(n_pairs=2, feat_off=bad), b"ascending"), (init, dict(cell=0), b"cell_size"),
                           (init, dict(scale=0.0), b"map_scale"), (init, dict(scale=float("nan")), b"map_scale"),
                           (init, dict(feat_off=np.array([1, 2], np.int32)), b"feat_off[0]"),
                           (tri, {}, b"null"), (tri, dict(n_pairs=-3), b"n_pairs"),
                           (tri, dict(n_pairs=2, feat_off=bad), b"ascending"), (tri, dict(feat_off=None), b"null")):
        assert call(**kw) == _capi.SVO_ERR_ARG, kw
        assert text in L.svo_last_error(), (kw, L.svo_last_error())


# ------------------------------------------------------------------ GPU
class _Got:
    pass


@pytest.fixture(scope="module")
def gpu_results():
    """Every batch through svo_amd.two_view_init_batch once; name -> that pair's outputs."""
    import svo_amd
    cam = svo_amd.PinholeCamera.kitti()
    out = {}
    for names in BATCHES:
        sc = [scene(k) for k in names]
        assert len({s.map_scale for s in sc}) == 1
        off = np.concatenate([[0], np.cumsum([s.n for s in sc])]).astype(np.int32)
        ref_px = np.ascontiguousarray(np.concatenate([s.ref_px for s in sc]).reshape(-1, 2))
        cur_px = np.ascontiguousarray(np.concatenate([s.cur_px for s in sc]).reshape(-1, 2))
        r = svo_amd.two_view_init_batch(cam, off, np.stack([s.E for s in sc]), np.stack([s.ref_pose for s in sc]),
                                        ref_px, cur_px, sc[0].map_scale, CELL)
        for p, k in enumerate(names):
            g = _Got()
            a, b = off[p], off[p + 1]
            g.F, g.counts, g.winner, g.cur_pose = r.F[p], r.counts[p], int(r.winner[p]), r.cur_poses[p]
            g.median_depth, g.n_valid = float(r.median_depth[p]), int(r.n_valid[p])
            g.ref_px, g.cur_px, g.points_world = ref_px[a:b], cur_px[a:b], r.points_world[a:b]
            g.valid, g.survivor, g.depth = r.valid[a:b], r.survivor[a:b], r.depth[a:b]
            out[k] = g
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", IN_BATCHES)
def test_gpu_two_view_init(name, gpu_results, tmp):
    check_pair(name, gpu_results[name], tmp)


@pytest.mark.gpu
def test_gpu_failed_pair_leaves_neighbours_intact(gpu_results, tmp):
    """The pair without matches fails (winner -1) inside a batch whose other pairs equal their restatements; a
    pair given on its own gives the same bits as inside that batch."""
    import svo_amd
    assert gpu_results["empty"].winner == -1
    for k in ("posed130", "forward257"):
        assert gpu_results[k].winner >= 0
        s = scene(k)
        rp, cp = s.ref_px.copy(), s.cur_px.copy()
        r = svo_amd.two_view_init_batch(svo_amd.PinholeCamera.kitti(), [0, s.n], s.E[None], s.ref_pose[None], rp, cp,
                                        s.map_scale, CELL)
        g = gpu_results[k]
        assert np.array_equal(r.points_world, g.points_world) and np.array_equal(r.cur_poses[0], g.cur_pose)
        assert np.array_equal(rp, g.ref_px) and np.array_equal(r.survivor, g.survivor)


@pytest.mark.gpu
def test_gpu_known_answer(gpu_results, tmp):
    """Zero pixel noise, identity reference pose, map_scale 1: every valid point lies on its reference ray, at one
    common multiple of its true depth, and the median of the current-camera depths is map_scale."""
    s, g = scene("exact257"), gpu_results["exact257"]
    ref = restated("exact257", tmp, F=np.ascontiguousarray(g.F))
    tol = C_POINT * EPS * ref.cond.max()
    v = np.nonzero(g.valid)[0]
    assert len(v) >= 0.9 * s.n
    X = g.points_world[v]
    ray = s.X_ref_true[v] / np.linalg.norm(s.X_ref_true[v], axis=1, keepdims=True)
    off_ray = np.linalg.norm(np.cross(X, ray), axis=1) / np.linalg.norm(X, axis=1)
    ratio = X[:, 2] / s.depth_true[v]
    Rg, tg = TV.pose_to_Rt(g.cur_pose)
    depth_cur = np.linalg.norm(g.points_world @ Rg.T + tg, axis=1)
    print("off-ray max", off_ray.max(), "scale spread", np.abs(ratio / ratio[0] - 1).max(), "median",
          TV.order_statistic_median(depth_cur), "tol", tol)
    assert off_ray.max() <= tol
    assert np.abs(ratio / ratio[0] - 1).max() <= tol
    assert abs(TV.reference_median(depth_cur, tmp)[2] / s.map_scale - 1) <= tol


@pytest.mark.gpu
def test_gpu_triangulate_dlt(tmp):
    """svo_triangulate_dlt alone: three pairs of unequal size, each with its own poses, against the restatement's
    triangulation within the per-match bound."""
    import svo_amd
    names = ["side65", "posed130", "side257"]
    K = TV.K_of()
    off, rps, cps, rpx, cpx, want, cond = [0], [], [], [], [], [], []
    for j, k in enumerate(names):
        s = scene(k)
        Rr, tr = TV.pose_to_Rt(s.ref_pose)
        Rc, tc = s.R_true @ Rr, s.R_true @ tr + s.t_true * (1.0 + 0.5 * j)
        X, c = TV.triangulate(K, Rr, tr, Rc, tc, s.ref_px, s.cur_px, want_cond=True)
        off.append(off[-1] + s.n)
        rps.append(s.ref_pose)
        cps.append(TV.Rt_to_pose(Rc, tc))
        rpx.append(s.ref_px)
        cpx.append(s.cur_px)
        # the poses the call sees are the 7-parameter ones: restate with exactly those
        Rc7, tc7 = TV.pose_to_Rt(cps[-1])
        X, c = TV.triangulate(K, Rr, tr, Rc7, tc7, s.ref_px, s.cur_px, want_cond=True)
        want.append(X)
        cond.append(c)
    got = svo_amd.triangulate_batch(svo_amd.PinholeCamera.kitti(), off, np.stack(rps), np.stack(cps),
                                    np.concatenate(rpx), np.concatenate(cpx))
    want, cond = np.concatenate(want), np.concatenate(cond)
    ratio = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1) / (EPS * cond)
    print("triangulate ratio max", ratio.max(), "cond max", cond.max())
    assert got.shape == (off[-1], 3) and np.all(ratio <= C_POINT)


def _frames(s, with_images=False):
    import svo_amd
    import svo_amd.synth as synth
    cam = svo_amd.PinholeCamera.kitti()
    if with_images:
        pair = synth.make_pair(n_features=60)
        imgs = (pair.ref_img, pair.cur_img, pair.kf_img)
    else:
        pair, imgs = None, (np.zeros((cam.height, cam.width), np.uint8),) * 3
    ref = svo_amd.Frame(cam, imgs[0], 5)
    cur = svo_amd.Frame(cam, imgs[1], 5)
    ref.abs_pose[:] = s.ref_pose
    ref.features = svo_amd.Feature._many(ref, s.ref_px)
    cur.features = svo_amd.Feature._many(cur, s.cur_px)
    return ref, cur, pair, imgs


@pytest.mark.gpu
def test_gpu_object_graph(gpu_results, tmp):
    """two_view_initialize on Frame / Feature / Point: the frames keep exactly the valid matches in order, each with
    one Point shared by its two features; the cached feature arrays follow; ImageAlignment runs on the result."""
    import svo_amd
    s, g = scene("posed130"), gpu_results["posed130"]
    ref, cur, pair, imgs = _frames(s, with_images=True)
    ref_feats, cur_feats = list(ref.features), list(cur.features)
    stale = ref.feature_arrays()[0]
    ok, median, n_points = svo_amd.two_view_initialize(ref, cur, s.E, s.map_scale, CELL)
    assert ok and median == g.median_depth and n_points == g.n_valid
    assert np.array_equal(cur.abs_pose, g.cur_pose)
    keep = np.nonzero(g.valid)[0]
    assert 0 < len(keep) < s.n  # the scene has matches to erase
    assert len(ref.features) == len(cur.features) == len(keep)
    assert all(a is ref_feats[i] and b is cur_feats[i] for a, b, i in zip(ref.features, cur.features, keep))
    for a, b in zip(ref.features, cur.features):
        assert a.point is not None and a.point is b.point and a.point.features == [a, b]
    assert all(ref_feats[i].point is None for i in np.nonzero(g.valid == 0)[0])
    for fr, px in ((ref, g.ref_px), (cur, g.cur_px)):
        apx, _, apt, ahp = fr.feature_arrays()
        assert apx is not stale and np.array_equal(apx, px[keep]) and np.array_equal(apt, g.points_world[keep])
        assert ahp.all()
    # the erased features kept their corrected pixels too (sampsonCorrection runs before anything is removed)
    assert all(np.array_equal(ref_feats[i].pixel_position, g.ref_px[i]) for i in range(s.n))
    # the map is usable by the rest of the project: sparse image alignment runs on it (no accuracy asserted)
    kf = svo_amd.Frame(ref.camera, imgs[2], 5)
    kf.abs_pose[:] = pair.kf_pose
    for i in range(pair.n_ref, len(pair.px)):
        kf.add_feature(svo_amd.Feature(kf, pair.px[i], bearing=pair.bearing[i], point=svo_amd.Point(pair.point[i])))
    ref.last_keyframe = kf
    err = svo_amd.ImageAlignment(5, 0, 4).align(ref, cur)
    assert np.isfinite(err) and np.isfinite(cur.abs_pose).all()


@pytest.mark.gpu
def test_gpu_failed_initialize_changes_pixels_only():
    """recoverPose fails (no matches in front of both cameras): two_view_initialize returns not-ok and touches
    nothing but the pixel positions (src/system.cpp:152-156)."""
    import svo_amd
    s = scene("empty")
    ref, cur, _, _ = _frames(s)
    pose = cur.abs_pose.copy()
    ok, median, n_points = svo_amd.two_view_initialize(ref, cur, s.E, MAP_SCALE, CELL)
    assert not ok and np.isnan(median) and n_points == 0 and np.array_equal(cur.abs_pose, pose)


@pytest.mark.gpu
def test_gpu_host_mirror(gpu_results, tmp):
    """host/svo.hpp initializeTwoView (build/svo_host_check init) on the same case: the same library call, so
    integers, pixels, pose and points are bit-equal to the Python path's."""
    s, g = scene("posed130"), gpu_results["posed130"]
    path = os.path.join(str(tmp), "init_case.bin")
    np.concatenate([[KITTI[k] for k in ("fx", "fy", "cx", "cy", "width", "height")], s.ref_pose, s.E.ravel(),
                    [s.map_scale, CELL, s.n], np.concatenate([s.ref_px, s.cur_px], axis=1).ravel()]).astype(np.float64).tofile(path)
    out = subprocess.run([HOST_CHECK, "init", path], capture_output=True, text=True, timeout=60, check=True).stdout
    lines = out.strip().split("\n")
    head = lines[0].split()
    assert head[0] == "init" and [int(x) for x in head[1:8]] == [1, g.winner, *g.counts.tolist(), g.n_valid]
    assert float(head[8]) == g.median_depth
    assert np.array_equal(np.array(lines[1].split()[1:], np.float64), g.cur_pose)
    rows = np.array([ln.split()[1:] for ln in lines[2:] if ln.startswith("pt ")], np.float64)
    tri = np.array([ln.split()[1:] for ln in lines[2:] if ln.startswith("tri ")], np.float64)
    keep = np.nonzero(g.valid)[0]
    assert rows.shape == (len(keep), 7)
    assert np.array_equal(rows[:, 0:2], g.ref_px[keep]) and np.array_equal(rows[:, 2:4], g.cur_px[keep])
    assert np.array_equal(rows[:, 4:7], g.points_world[keep])
    # algorithm::triangulate3DWorldPoints of the mirror on the initialised frames = triangulate_batch on the same input
    import svo_amd
    want = svo_amd.triangulate_batch(svo_amd.PinholeCamera.kitti(), [0, len(keep)], s.ref_pose[None], g.cur_pose[None],
                                     g.ref_px[keep], g.cur_px[keep])
    assert np.array_equal(tri, want)
