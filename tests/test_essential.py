"""svo_essential_ransac / svo_essential_score (include/svo_c.h "essential-matrix RANSAC") against the numpy restatement
of the contract (tests/essential_ref.py), the restatement against scenes of known motion, the conditions that make the
GPU comparison complete, and the frame-level mirrors of algorithm::computeEssentialMatrix (Python and C++)."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import essential_ref as R
import two_view_ref as T
import svo_amd
from svo_amd import _capi, _paths
from common import KITTI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured by the CPU tests below (each prints its figure), on the committed scenes:
# the largest difference between a model of the restatement (SVD null space) and of its second opinion (eigh of the
# Gram matrix) over every committed sample.  The GPU's models must agree with the restatement's within 8 x this.
METHOD_DIFF = 1.31e-9
MODEL_TOL = 8 * METHOD_DIFF
# the largest scaled residual of the ten constraints over the restatement's models; the GPU's within 8 x this
REF_RESIDUAL = 2.5e-16
# |E - E_true / |E_true||, noise-free general scene, of the restatement (float32 pixels through a minimal sample)
TRUTH_ERR = 6.7e-5
# the restatement's chain (RANSAC, then the two-view initialisation) on the noisy scene: rotation error (rad) and
# the angle between the translation directions (rad)
CHAIN_ROT, CHAIN_DIR = 5.4e-4, 8.0e-2

SCENE_NAMES = list(R.SCENES)


def _cam():
    return svo_amd.PinholeCamera.kitti()


def _unclear(run):
    return [h for h, s in enumerate(run.samples) if s is not None and not s.clear]


# ---------------------------------------------------------------- the generator
def test_sampler_draws_are_in_range_and_distinct():
    for n in (5, 6, 64, 2000):
        for h in range(50):
            idx = R.sample(12345, 3, h, n)
            assert idx is not None and len(set(idx)) == 5 and all(0 <= i < n for i in idx)
    assert R.sample(1, 0, 0, 4) is None  # four matches: never five distinct indices


def test_sampler_pinned_table():
    """mix() against the published splitmix64 stream (seed 0: the first outputs of the generator are mix(0),
    mix(0x9E37..15), ...) and the first samples of (seed 7, pair 2, n 100)."""
    assert R.mix(0) == 0xE220A8397B1DCDAF
    assert R.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    got = [R.sample(7, 2, h, 100) for h in range(4)]
    for h, idx in enumerate(got):  # restated with plain integers
        want, c = [], 0
        while len(want) < 5:
            z = (7 ^ (2 << 44) ^ (h << 8) ^ c) & R.MASK64
            v = ((R.mix(z) >> 32) * 100) >> 32
            if v not in want:
                want.append(v)
            c += 1
        assert idx == want
    assert got == PINNED_SAMPLES


PINNED_SAMPLES = [[71, 89, 50, 1, 3], [49, 9, 21, 81, 97], [95, 72, 75, 70, 15], [37, 25, 41, 50, 47]]


def test_sampler_depends_on_seed_and_pair():
    base = [R.sample(7, 0, h, 500) for h in range(8)]
    assert base != [R.sample(8, 0, h, 500) for h in range(8)]
    assert base != [R.sample(7, 1, h, 500) for h in range(8)]
    assert len({tuple(s) for s in base}) == 8


# ---------------------------------------------------------------- the solver
def test_solver_models_satisfy_their_equations():
    """Every model of every committed sample: the five epipolar equations and the ten constraints.  Measured largest
    values: epipolar 6.0e-16, constraints (scaled) 2.41e-16."""
    epi = res = 0.0
    count = 0
    for name in SCENE_NAMES:
        for s in R.scene_run(name).samples:
            if s is None or len(s.models) == 0:
                continue
            count += len(s.models)
            epi = max(epi, float(s.epipolar.max()))
            res = max(res, max(R.constraint_residual(m) for m in s.models))
            assert np.allclose(np.linalg.norm(s.models.reshape(-1, 9), axis=1), 1.0, rtol=0, atol=1e-15)
    print(f"{count} models: largest epipolar residual {epi:.3e}, largest scaled constraint residual {res:.3e}")
    assert count > 1000
    assert epi <= 1e-14 and res <= REF_RESIDUAL


def test_two_null_space_methods_agree():
    """The measured tolerance of the GPU comparison: SVD against eigh-of-the-Gram null spaces over every committed
    sample (clear ones; the others are counted).  Measured: 1.303e-9 (a sample of the planar scene; 1.67e-10 without it)."""
    worst, unclear, total = 0.0, 0, 0
    for name in SCENE_NAMES:
        a, b = R.scene_run(name), R.scene_run(name, "eigh")
        assert a.iterations == b.iterations and a.best[0] == b.best[0] and a.n_inliers == b.n_inliers
        assert np.array_equal(a.mask, b.mask)
        for x, y in zip(a.samples, b.samples):
            total += 1
            if not (x.clear and y.clear):
                unclear += 1
                continue
            d = R.match_models(x.models, y.models)
            assert math.isfinite(d), name
            worst = max(worst, d)
    print(f"{total} samples, {unclear} unclear, largest model difference between the methods {worst:.3e}")
    assert worst <= METHOD_DIFF and unclear <= 0.02 * total


# ---------------------------------------------------------------- truth
def test_truth_general_scene():
    """200 noise-free matches, 30 % outliers: every true inlier is in the mask and E is the true one within twice the
    restatement's own error (measured 6.63e-5: the float32 pixels through the winner's minimal sample)."""
    s, r = R.scene("general"), R.scene_run("general")
    assert r.status == 0 and (r.mask[s.inlier] == 1).all()
    Et = s.E / np.linalg.norm(s.E)
    err = min(np.abs(r.E - Et).max(), np.abs(r.E + Et).max())
    print(f"general scene: |E - E_true| = {err:.3e}, {r.n_inliers} inliers, {r.iterations} samples")
    assert err <= 2 * TRUTH_ERR


def test_truth_planar_scene():
    """Coplanar points admit a second essential matrix, so only the inliers are asked for."""
    s, r = R.scene("planar"), R.scene_run("planar")
    assert r.status == 0 and (r.mask[s.inlier] == 1).all()
    x1, x2 = R.normalise(s.ref_px), R.normalise(s.cur_px)
    assert (R.sampson_err(r.E, x1, x2)[s.inlier] <= R.thr2_of(1.0)).all()


# ---------------------------------------------------------------- conditions on every committed (scene, seed)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_committed_scene_conditions(name):
    r = R.scene_run(name)
    print(f"{name}: {r.iterations} samples, margin {r.margin:.3e}, {r.diag}, unclear {_unclear(r)}")
    assert r.margin > 1e-6            # no Sampson decision within 1e-6 relative of thr2
    assert r.diag["half_integer_margin"] > 1e-6
    if R.SCENES[name][1] > 5:         # with five matches every model of the one sample fits all five: the tie is
        assert r.diag["ties"] == 0    # inherent, and the GPU test of that scene does not compare the winner's k
    assert len(_unclear(r)) <= 0.02 * len(r.samples)


def test_stopping_rule():
    assert R.scene_run("one").iterations == 1
    assert R.scene_run("half").iterations > R.scene_run("fifth").iterations
    assert R.update_iterations(0.999, 0.0, 1000)[0] == 0
    assert R.update_iterations(0.999, 1.0, 1000)[0] == 1000
    assert R.update_iterations(0.999, 0.3, 1000)[0] == int(np.rint(math.log(0.001) / math.log(1 - 0.7 ** 5)))


# ---------------------------------------------------------------- C ABI (no device)
def test_abi_exports_and_signatures():
    c_void_p, c_int32, c_double, c_uint64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64
    cam = ctypes.POINTER(_capi.SvoCamera)
    assert "svo_essential_ransac" in _capi.EXPORTED and "svo_essential_score" in _capi.EXPORTED
    L = _capi.lib()
    assert list(L.svo_essential_score.argtypes) == [c_void_p, cam, c_int32] + [c_void_p] * 5 + [c_double, c_void_p, c_void_p]
    assert list(L.svo_essential_ransac.argtypes) == ([c_void_p, cam, c_int32, c_void_p, c_void_p, c_void_p, c_double,
                                                      c_double, c_int32, c_uint64] + [c_void_p] * 8)
    src = open(os.path.join(ROOT, "include", "svo_c.h")).read()
    decl = src[src.index("int svo_essential_ransac("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int svo_essential_ransac(svo_ctx* ctx, const svo_camera* cam, int32_t n_pairs, "
                    "const int32_t* feat_off, const double* ref_px, const double* cur_px, double threshold, "
                    "double confidence, int32_t max_iterations, uint64_t seed, double* E, uint8_t* mask, "
                    "int32_t* n_inliers, int32_t* iterations, int32_t* best, int32_t* status, double* hyp_E, "
                    "int32_t* hyp_count)")
    assert L.svo_abi_version() == 2


@pytest.mark.parametrize("thr,conf,iters,off,what", [
    (0.0, 0.999, 1000, [0, 8], b"threshold"), (-1.0, 0.999, 1000, [0, 8], b"threshold"),
    (1.0, 0.0, 1000, [0, 8], b"confidence"), (1.0, 1.0, 1000, [0, 8], b"confidence"),
    (1.0, 0.999, 0, [0, 8], b"max_iterations"), (1.0, 0.999, 65537, [0, 8], b"max_iterations"),
    (1.0, 0.999, 1000, [0, 8, 6], b"ascending")])
def test_abi_rejects_arguments_before_the_context(thr, conf, iters, off, what):
    """All handles NULL: no device exists on this path."""
    off = np.array(off, np.int32)
    L = _capi.lib()
    assert L.svo_essential_ransac(None, None, len(off) - 1, _capi.ptr(off), None, None, thr, conf, iters, 0, None, None,
                                  None, None, None, None, None, None) == _capi.SVO_ERR_ARG
    assert what in L.svo_last_error()
    if what in (b"threshold", b"ascending"):
        assert L.svo_essential_score(None, None, len(off) - 1, _capi.ptr(off), _capi.ptr(off), None, None, None, thr,
                                     None, None) == _capi.SVO_ERR_ARG
        assert what in L.svo_last_error()


def test_abi_rejects_null_handles():
    off = np.array([0, 8], np.int32)
    L = _capi.lib()
    assert L.svo_essential_ransac(None, None, 1, _capi.ptr(off), None, None, 1.0, 0.999, 1000, 0, None, None, None, None,
                                  None, None, None, None) == _capi.SVO_ERR_ARG
    assert b"null" in L.svo_last_error()


def test_kernels_use_no_private_segment():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "essential.o"))
    assert len(res) >= 5 and any("solve" in k for k in res)
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name


# ---------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _gpu_run(name, seed_offset=0):
    s = R.scene(name)
    return svo_amd.essential_ransac_batch(_cam(), [0, s.n], s.ref_px, s.cur_px, 1.0, 0.999, R.SCENES[name][6],
                                          R.SCENES[name][5] + seed_offset, trace=True)


def _check_pair(g, p, ref_px, cur_px, want, max_it, compare_k=True, first=0):
    """Pair p of a traced GPU result (its matches start at `first`) against the restatement's run `want` of the same
    matches."""
    n = len(ref_px)
    own = slice(first, first + n)
    x1, x2 = R.normalise(ref_px), R.normalise(cur_px)
    thr2 = R.thr2_of(1.0)
    it = int(g.iterations[p])
    hc, hE = g.hyp_count[p], g.hyp_E[p]
    # trace, scoring: the counts are the restatement's scoring of the returned models, exactly
    assert (hc[it:] == -2).all() and (hE[it:] == 0).all()
    for h in range(it):
        k = int((hc[h] >= 0).sum())
        assert (hc[h, :k] >= 0).all() and (hc[h, k:] == -1).all() and (hE[h, k:] == 0).all()
        for j in range(k):
            assert hc[h, j] == int(np.count_nonzero(R.inliers(hE[h, j], x1, x2, thr2))), (h, j)
    # outcome: the sequential rule on the GPU's own counts, exactly
    w_it, w_best, w_inl, _ = R.walk(hc, n, 0.999, max_it)
    assert (it, tuple(g.best[p]), int(g.n_inliers[p])) == (w_it, w_best, w_inl)
    assert np.array_equal(g.E[p], hE[w_best[0], w_best[1]])
    assert np.array_equal(g.mask[own], R.inliers(g.E[p], x1, x2, thr2).astype(np.uint8))
    # ... and the restatement's full run
    assert it == want.iterations and int(g.n_inliers[p]) == want.n_inliers and g.status[p] == want.status
    assert int(g.best[p][0]) == want.best[0]
    assert np.array_equal(g.mask[own], want.mask)
    assert min(np.abs(g.E[p] - want.E).max(), np.abs(g.E[p] + want.E).max()) <= MODEL_TOL or not compare_k
    # trace, solution sets on the clear samples
    worst = res = 0.0
    skipped = 0
    for h in range(it):
        s = want.samples[h]
        k = int((hc[h] >= 0).sum())
        for j in range(k):
            res = max(res, R.constraint_residual(hE[h, j]))
        if s is None:
            assert k == 0
            continue
        if not s.clear:
            skipped += 1
            continue
        d = R.match_models(hE[h, :k], s.models)
        assert math.isfinite(d), (h, k, len(s.models))
        worst = max(worst, d)
    print(f"pair {p}: {it} samples, {skipped} unclear, largest model difference {worst:.3e}, largest residual {res:.3e}")
    assert skipped <= 0.02 * max(it, 1) or skipped == 0
    assert worst <= MODEL_TOL and res <= 8 * REF_RESIDUAL


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_gpu_scene_matches_restatement(name):
    s = R.scene(name)
    g = _gpu_run(name)
    _check_pair(g, 0, s.ref_px, s.cur_px, R.scene_run(name), R.SCENES[name][6], compare_k=s.n > 5)
    if s.n == 5:  # the tie among the exact models of the one sample: the winner is one of the restatement's models
        assert min(min(np.abs(g.E[0] - m).max(), np.abs(g.E[0] + m).max()) for m in R.scene_run(name).samples[0].models) <= MODEL_TOL


@pytest.mark.gpu
def test_gpu_four_matches_have_no_model():
    s = R.scene("n6")
    g = svo_amd.essential_ransac_batch(_cam(), [0, 4], s.ref_px[:4], s.cur_px[:4], trace=True)
    assert g.status[0] == -1 and g.iterations[0] == 0 and g.n_inliers[0] == 0 and tuple(g.best[0]) == (-1, -1)
    assert not g.E.any() and not g.mask.any() and (g.hyp_count == -2).all() and not g.hyp_E.any()


@pytest.mark.gpu
def test_gpu_batch_of_unequal_pairs_with_an_empty_one():
    a, b = R.scene("n63"), R.scene("n257")
    off = [0, a.n, a.n, a.n + b.n]
    ref_px, cur_px = np.concatenate([a.ref_px, b.ref_px]), np.concatenate([a.cur_px, b.cur_px])
    g = svo_amd.essential_ransac_batch(_cam(), off, ref_px, cur_px, 1.0, 0.999, 1000, 77, trace=True)
    assert g.status[1] == -1 and g.iterations[1] == 0 and not g.E[1].any() and (g.hyp_count[1] == -2).all()
    for p, s in ((0, a), (2, b)):
        want = R.ransac(s.ref_px, s.cur_px, 1.0, 0.999, 1000, 77, pair=p)
        assert want.margin > 1e-6 and want.diag["ties"] == 0 and want.diag["half_integer_margin"] > 1e-6
        _check_pair(g, p, s.ref_px, s.cur_px, want, 1000, first=off[p])
    # the untraced call returns the same bytes
    u = svo_amd.essential_ransac_batch(_cam(), off, ref_px, cur_px, 1.0, 0.999, 1000, 77)
    for f in ("E", "mask", "n_inliers", "iterations", "best", "status"):
        assert getattr(u, f).tobytes() == getattr(g, f).tobytes(), f


@pytest.mark.gpu
def test_gpu_two_runs_give_equal_bytes_and_seeds_differ():
    s = R.scene("n257")
    one = _gpu_run("n257")
    two = svo_amd.essential_ransac_batch(_cam(), [0, s.n], s.ref_px, s.cur_px, 1.0, 0.999, 1000, R.SCENES["n257"][5],
                                         trace=True)
    for f in ("E", "mask", "n_inliers", "iterations", "best", "status", "hyp_E", "hyp_count"):
        assert getattr(one, f).tobytes() == getattr(two, f).tobytes(), f
    other = _gpu_run("n257", 1)
    assert other.hyp_E[0, 0].tobytes() != one.hyp_E[0, 0].tobytes()


SCORE_CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, width=640, height=480)


@pytest.mark.gpu
def test_gpu_score_matches_restatement_exactly():
    """Given models: the winner and three other models of a scene, a model with a NaN entry, and (second pair) the
    pure forward translation E = [e_z]x with a match on both epipoles (den = 0) and one on the threshold's far side."""
    s, r = R.scene("n257"), R.scene_run("n257")
    models = [r.E] + [m for smp in r.samples[:3] for m in smp.models[:1]]
    bad = r.E.copy()
    bad[1, 2] = np.nan
    models.append(bad)
    x1, x2 = R.normalise(s.ref_px), R.normalise(s.cur_px)
    thr2 = R.thr2_of(1.0)
    counts, mask = svo_amd.essential_score_batch(_cam(), [0, s.n], [0, len(models)], np.stack(models), s.ref_px, s.cur_px)
    want = [int(np.count_nonzero(R.inliers(m, x1, x2, thr2))) for m in models]
    assert counts.tolist() == want and want[-1] == 0 and want[0] == r.n_inliers
    assert np.array_equal(mask, R.inliers(models[int(np.argmax(want))], x1, x2, thr2).astype(np.uint8))
    # the epipole
    cam = svo_amd.PinholeCamera(640, 480, 500.0, 500.0, 320.0, 240.0)
    Ez = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    ref = np.array([[320.0, 240.0], [400.0, 300.0], [100.0, 50.0], [320.0, 240.0]])
    cur = np.array([[320.0, 240.0], [480.0, 360.0], [120.0, 47.0], [330.0, 250.0]])
    y1, y2 = R.normalise(ref, SCORE_CAM), R.normalise(cur, SCORE_CAM)
    t2 = R.thr2_of(1.0, SCORE_CAM)
    assert np.isnan(R.sampson_err(Ez, y1, y2)[0])  # 0 / 0 on the epipoles
    counts, mask = svo_amd.essential_score_batch(cam, [0, 0, 4], [0, 0, 2], np.stack([Ez, -Ez]), ref, cur)
    want = R.inliers(Ez, y1, y2, t2)
    assert want.tolist() == [False, True, False, True]
    assert counts.tolist() == [2, 2] and np.array_equal(mask, want.astype(np.uint8))


# ---------------------------------------------------------------- frame level
def _frames(s):
    cam = _cam()
    img = np.zeros((KITTI["height"], KITTI["width"]), np.uint8)
    ref, cur = svo_amd.Frame(cam, img, 1), svo_amd.Frame(cam, img, 1)
    ref.features = svo_amd.Feature._many(ref, s.ref_px)
    cur.features = svo_amd.Feature._many(cur, s.cur_px)
    return ref, cur


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["above", "below"])
def test_gpu_compute_essential_matrix(side):
    s = R.scene("general")
    want = R.ransac(s.ref_px, s.cur_px, 1.0, 0.999, 1000, 5)
    assert want.margin > 1e-6 and want.diag["ties"] == 0 and want.diag["half_integer_margin"] > 1e-6
    ref, cur = _frames(s)
    before = (list(ref.features), list(cur.features))
    versions = (ref._feat_ver[0], cur._feat_ver[0])
    thr = want.n_inliers - 1 if side == "above" else want.n_inliers
    ok, E = svo_amd.compute_essential_matrix(ref, cur, 1.0, thr, seed=5)
    assert ok == (side == "above")
    assert min(np.abs(E - want.E).max(), np.abs(E + want.E).max()) <= MODEL_TOL
    for fr, old in zip((ref, cur), before):
        kept = [f for f, k in zip(old, want.mask) if k]
        assert len(fr.features) == len(kept) and all(x is y for x, y in zip(fr.features, kept))
    assert (ref._feat_ver[0], cur._feat_ver[0]) == (versions[0] + 1, versions[1] + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["above", "below"])
def test_gpu_host_mirror_compute_essential_matrix(side, tmp_path):
    """svo_amd::algorithm::computeEssentialMatrix through `svo_host_check essential`: the same bits as the Python path."""
    s = R.scene("general")
    ref, cur = _frames(s)
    ok_py, E_py = svo_amd.compute_essential_matrix(ref, cur, 1.0, 0, seed=5)
    n_in = ref.number_observation()
    thr = n_in - 1 if side == "above" else n_in
    head = [KITTI["fx"], KITTI["fy"], KITTI["cx"], KITTI["cy"], KITTI["width"], KITTI["height"], 1.0, thr, 5, s.n]
    np.concatenate([np.array(head, np.float64), np.concatenate([s.ref_px, s.cur_px], axis=1).ravel()]).tofile(tmp_path / "e.bin")
    out = subprocess.run([_paths.lib_path("svo_host_check"), "essential", str(tmp_path / "e.bin")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    head = lines[0].split()
    assert head[0] == "essential" and int(head[1]) == (1 if side == "above" else 0)
    assert int(head[2]) == n_in and int(head[3]) == n_in
    E = np.array([float.fromhex(v) for v in lines[1].split()[1:]]).reshape(3, 3)
    assert E.tobytes() == E_py.tobytes()

    def rows(tag):
        return np.array([[float.fromhex(v) for v in ln.split()[1:]] for ln in lines if ln.startswith(tag + " ")]).reshape(-1, 2)
    for tag, fr in (("ref", ref), ("cur", cur)):
        assert rows(tag).tobytes() == np.array([f.pixel_position for f in fr.features]).reshape(-1, 2).tobytes()


@pytest.mark.gpu
def test_gpu_chain_recovers_the_motion(tmp_path):
    """compute_essential_matrix, then two_view_initialize, on a noisy scene with outliers: the true rotation and
    translation direction within twice what the restatement's chain shows (measured there: rotation 5.37e-4 rad,
    direction 7.97e-2 rad)."""
    s = R.scene("n257")

    def errors(R_est, t_est):
        dR = R_est @ s.R_true.T
        rot = math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0)))
        c = float(t_est @ s.t_true) / (np.linalg.norm(t_est) * np.linalg.norm(s.t_true))
        return rot, math.acos(min(1.0, max(-1.0, c)))
    want = R.scene_run("n257")
    keep = want.mask == 1
    rr = T.two_view_init(want.E, T.IDENTITY, s.ref_px[keep].copy(), s.cur_px[keep].copy(), 1.0, 30, tmp_path)
    ref_rot, ref_dir = errors(rr.cur_R, rr.cur_t)
    print(f"restatement chain: rotation error {ref_rot:.3e} rad, direction error {ref_dir:.3e} rad")
    assert ref_rot <= CHAIN_ROT and ref_dir <= CHAIN_DIR
    ref, cur = _frames(s)
    ok, E = svo_amd.compute_essential_matrix(ref, cur, 1.0, 50, seed=R.SCENES["n257"][5])
    assert ok
    ok, _, n_points = svo_amd.two_view_initialize(ref, cur, E, 1.0, 30)
    assert ok and n_points > 100
    Rg, tg = T.pose_to_Rt(cur.abs_pose)
    rot, dr = errors(Rg, tg)
    print(f"GPU chain: rotation error {rot:.3e} rad, direction error {dr:.3e} rad")
    assert rot <= 2 * CHAIN_ROT and dr <= 2 * CHAIN_DIR
