"""The tracker itself: System::addImage from images to a trajectory (src/system.cpp:15-511 of the reference).

CPU (not gpu): the restatement (tests/system_ref.py, the System over the CPU checkers) on the synthetic band sequence
(tests/system_scene.py): the state machine's path, the keyframe rule, seeds -> candidates -> features, the eviction
path, the failure paths, and the cap on borderline decisions: no floating-point decision of the committed scene lies
closer than 1e-6 (relative) to its threshold, so the GPU run may differ from the restatement in no decision.

Trajectory against ground truth, after the one free scale (least squares over the camera centres): the largest
position error over the eight frames is 0.006 steps (0.009 in the eviction variant); asserted below 0.05 steps, the
camera displacement that moves the nearest band (20 px per step) by one pixel.

GPU: svo_amd.System on the same frames against the restatement, frame by frame: result, status, keyframe flag, number
of observations, observations with points, seeds, candidates, keyframes and the features the bundle adjustments removed
are compared exactly, absPose within POSE_BOUND.  MEASURED_POSE_DIFF is the largest GPU-versus-restatement difference
of a pose parameter over both sequences on an MI355X; the bound is ten times that (run-to-run libm differences the
components already document), and never above 1e-6, a tenth of the project's 1e-5 pose bar.  The relocalisation
branch, entered through the setter, equals one ImageAlignment.align against getClosestKeyframe's frame.

GPU, the two mirrors: svo_amd::System (build/svo_host_check system) against svo_amd.System on the eight frames, the
eviction variant and a relocalisation at the last frame: discrete fields equal, poses and trajectory text bitwise.
"""
import functools
import io
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import system_ref as SR
import system_scene as SC
from common import canon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "build", "svo_host_check")
MEASURED_POSE_DIFF = 4.224e-11
POSE_BOUND = min(10.0 * MEASURED_POSE_DIFF, 1e-6)
EXACT = ("result", "status", "keyframe", "n_obs", "n_obs_points", "seeds", "candidates", "keyframes", "ba_removed")


def sequence(n_frames=SC.N_FRAMES):
    return _sequence(int(n_frames))


@functools.lru_cache(maxsize=None)
def _sequence(n_frames):
    imgs, gt = SC.make_sequence(n_frames)
    imgs.flags.writeable = False
    gt.flags.writeable = False
    return imgs, gt


def restatement(max_keyframes=7, n_frames=SC.N_FRAMES, relocalise=False):
    """(system, records) of the restatement; computed once and shared (nobody modifies it)."""
    return _restatement(int(max_keyframes), int(n_frames), bool(relocalise))


@functools.lru_cache(maxsize=None)
def _restatement(max_keyframes, n_frames, relocalise):
    imgs, _ = sequence(n_frames)
    return SR.run(imgs, SR.Config(**SC.config_kwargs(max_keyframes=max_keyframes)), relocalise)


def trajectory_error(poses, gt):
    """Largest position error in steps after the least-squares scale over the camera centres."""
    C = np.array([SR.camera_in_world(p) for p in poses])
    G = np.array([SR.camera_in_world(p) for p in gt])
    s = (C * G).sum() / (C * C).sum()
    return float(np.abs(s * C - G).max()) / SC.STEP


# ---------------------------------------------------------------- CPU: the restatement on the scene
def test_scene_is_exact_and_textured():
    import svo_amd.synth as synth
    imgs, gt = sequence()
    edges = [SC.HEIGHT * b // 4 for b in range(5)]
    for b, d in enumerate(SC.DISPARITY):
        band = imgs[:, edges[b]:edges[b + 1]]
        assert np.array_equal(band[3][:, :SC.WIDTH - 3 * d], band[0][:, 3 * d:])  # a pure integer shift
        assert float(d) == SC.FX * SC.STEP / SC.band_depths()[b]
    assert synth.gradient_fraction(imgs[0], 50) > 0.5
    assert np.array_equal(SR.camera_in_world(gt[3]), [3 * SC.STEP, 0, 0])


def test_state_machine_path():
    s, recs = restatement()
    assert [r["status"] for r in recs] == [SR.SECOND] + [SR.NEW] * 7          # first -> second -> new
    assert [r["result"] for r in recs] == [SR.SUCCESS] * 4 + [SR.KEYFRAME] + [SR.SUCCESS] * 2 + [SR.KEYFRAME]
    # frames 0 and 1 are keyframes; the next one is the first frame with diffId >= 3 (4 - 1), then 7 - 4
    assert [r["keyframe"] for r in recs] == [True, True, False, False, True, False, False, True]
    assert s.events["local_ba"] == [4, 7]                                    # localBA ran exactly there
    assert [r["keyframes"] for r in recs] == [1, 2, 2, 2, 3, 3, 3, 4]
    assert recs[1]["seeds"] > 0 and recs[0]["seeds"] == 0                     # seeds exist after frame 1
    assert s.events["seeds_converged"] >= 1 and s.events["candidates_added"] >= 1
    assert all(r["n_obs"] >= 50 for r in recs)                               # tracking quality never failed


@pytest.mark.parametrize("max_keyframes,n_frames,relocalise", [(7, 8, False), (2, 9, False), (2, 9, True)])
def test_no_borderline_decision(max_keyframes, n_frames, relocalise):
    s, recs = restatement(max_keyframes, n_frames, relocalise)
    names = ["error < 50", "chi2 > 4", "sqrt(var) * 10 < maxDepth", "disparity", "sampson", "in frame (3 px)",
             "two-view validity", "in frame (5 px)"]
    if relocalise:  # isVisible is reached only through getCloseKeyframes
        names.append("in frame (isVisible)")
        assert recs[-1]["status"] == SR.RELOCALIZATION and recs[-1]["result"] == SR.SUCCESS
    for name in names:
        assert name in s.margins, name                                       # every kind of decision was met
    print({k: "%.2e" % v for k, v in s.margins.items()})
    assert min(s.margins.values()) >= SR.CAP, s.margins


@pytest.mark.parametrize("max_keyframes,n_frames", [(7, 8), (2, 9)])
def test_trajectory_against_ground_truth(max_keyframes, n_frames):
    _, recs = restatement(max_keyframes, n_frames)
    _, gt = sequence(n_frames)
    err = trajectory_error([r["pose"] for r in recs], gt)
    print("largest position error: %.4f steps" % err)
    assert err < 0.05


def test_eviction_path():
    s, recs = restatement(2, 9)
    ref, _ = restatement(7, 9)
    assert s.events["evicted"] == [0, 1]                                     # at keyframes 4 and 7: the furthest
    assert [r["keyframes"] for r in recs] == [1, 2, 2, 2, 2, 2, 2, 2, 2]
    base = s.cur.id - 8
    assert sorted(k.id - base for k in s.key_frames) == [4, 7]
    # keyframe 1 owned seeds when it was evicted (frame 7); they left at the next update (frame 8)
    owned = [f.frame.id - (ref.cur.id - 8) for f in ref.seed_features]
    assert 1 in owned and all(f.frame.id - base != 1 for f in s.seed_features)
    assert len(s.seeds) == len(s.seed_features) < len(ref.seeds)
    assert all(0 <= k < len(s.seed_keyframes) for k in s.seeds["kf"])
    assert all(s.seed_keyframes[k] is f.frame for k, f in zip(s.seeds["kf"], s.seed_features))
    for fr in s.key_frames + [s.ref, s.cur]:
        for f in fr.features:
            assert f.point is None or f.point.type != SR.DELETED
            assert f.point is None or all(g.frame.id - base not in (0, 1) for g in f.point.features)
    assert all(cd[0].frame.id - base not in (0, 1) for cd in s.candidates)


def test_blank_first_image_fails():
    s = SR.System(SR.Config(**SC.config_kwargs()))
    assert s.add_image(np.full((SC.HEIGHT, SC.WIDTH), 128, np.uint8), 0) is False
    assert s.status == SR.FIRST and s.ref is None and not s.key_frames


def test_identical_second_image_fails_on_disparity_then_initialises():
    imgs, _ = sequence()
    _, recs = restatement()
    s = SR.System(SR.Config(**SC.config_kwargs()))
    assert s.add_image(imgs[0], 0) is True
    first = s.ref
    assert s.add_image(imgs[0], 1) is False                                  # median disparity 0 < threshold
    assert s.status == SR.SECOND and s.ref is first and s.margins["disparity"] == 1.0
    assert s.add_image(imgs[1], 2) is True                                   # the third image against the first
    assert s.status == SR.NEW and len(s.key_frames) == 2 and s.key_frames[0] is first
    assert np.array_equal(s.cur.pose, recs[1]["pose"]) and s.cur.n_obs() == recs[1]["n_obs"]


def _adversary(n):
    """McIlroy's quicksort adversary against the library's own nth_element (comparisons through __lt__): a
    permutation of 0..n-1 on which median-of-three introselect degenerates, so the heap-select branch runs."""
    import svo_amd.core as core
    gas = n
    state = dict(solid=0, cand=None)
    val = [gas] * n

    class Item:
        def __init__(self, i):
            self.i = i

        def __lt__(self, other):
            a, b = self.i, other.i
            if val[a] == gas and val[b] == gas:
                k = a if a == state["cand"] else b
                val[k] = state["solid"]
                state["solid"] += 1
            if val[a] == gas:
                state["cand"] = a
            elif val[b] == gas:
                state["cand"] = b
            return val[a] < val[b]

    core._nth_element([Item(i) for i in range(n)], n // 2)
    rest = [i for i in range(n) if val[i] == gas]
    for i in rest:
        val[i] = state["solid"]
        state["solid"] += 1
    return np.array(val, np.float64)


def test_host_median_is_the_toolchains_nth_element():
    """svo_amd.compute_median (a restatement of libstdc++'s introselect, including its heap-select branch) against
    algorithm::computeMedian over the real std::nth_element (the oracle's)."""
    import svo_amd
    rng = np.random.default_rng(5)
    cases = [rng.random(n) for n in (1, 2, 3, 4, 5, 8, 33, 84, 85, 200, 1000, 1001, 4096)]
    cases += [np.floor(rng.random(n) * 7) for n in (10, 64, 501)]           # heavy duplicates
    cases += [np.arange(64.0), np.arange(65.0)[::-1].copy(), np.zeros(16)]
    cases += [_adversary(n) for n in (64, 200, 1024)]
    for v in cases:
        assert svo_amd.compute_median(v) == O.median(v, len(v)), len(v)
    assert math.isnan(svo_amd.compute_median([]))


def test_host_pose_algebra():
    import svo_amd
    rng = np.random.default_rng(9)
    for _ in range(8):
        a, b = (O.se3_exp(rng.normal(size=6)) for _ in range(2))
        assert np.abs(canon(svo_amd.pose_compose(a, b)) - canon(O.se3_compose(a, b))).max() < 1e-14
        assert np.abs(canon(svo_amd.pose_inverse(a)) - canon(SR.pose_inverse(a))).max() < 1e-14
        assert np.abs(canon(svo_amd.pose_compose(a, svo_amd.pose_inverse(a))) - SR.IDENTITY).max() < 1e-14


# ---------------------------------------------------------------- GPU: svo_amd.System against the restatement
def gpu_run(images, **over):
    import svo_amd
    system = svo_amd.System(svo_amd.Config(**SC.config_kwargs(**over)), instrument=True)
    base = svo_amd.Frame._frame_counter
    recs, lines = [], io.StringIO()
    for k, img in enumerate(images):
        ok = system.add_image(img, k)
        cur = system.cur_frame
        assert ok == (system.last_result != svo_amd.System.FAILED)
        recs.append(dict(result=system.last_result, status=system.status, keyframe=cur.is_keyframe(),
                         n_obs=cur.number_observation(), n_obs_points=cur.number_observation_with_points(),
                         seeds=system.depth_estimator.number_filters(), candidates=len(system.map.candidates),
                         keyframes=system.map.size_keyframes(),
                         ba_removed=sorted((f - base, i) for f, i in system.ba_removed),
                         pose=np.array(cur.abs_pose, np.float64)))
        system.write_in_file(lines)
    return system, recs, lines.getvalue()


def compare(recs, want):
    worst = 0.0
    for k, (g, c) in enumerate(zip(recs, want)):
        for name in EXACT:
            assert g[name] == c[name], (k, name, g[name], c[name])
        worst = max(worst, float(np.abs(canon(g["pose"]) - canon(c["pose"])).max()))
    print("largest pose-parameter difference GPU vs restatement: %.3e" % worst)
    assert worst <= POSE_BOUND, worst
    return worst


@pytest.mark.gpu
def test_gpu_system_matches_restatement():
    import svo_amd
    imgs, gt = sequence()
    _, want = restatement()
    system, recs, text = gpu_run(imgs)
    compare(recs, want)
    assert trajectory_error([r["pose"] for r in recs], gt) < 0.05
    # the trajectory text: System.write_in_file is trajectory.write_in_file over the same poses, byte for byte
    import svo_amd.trajectory as trajectory

    class Posed:
        pass

    out = io.StringIO()
    for r in recs:
        fr = Posed()
        fr.abs_pose = r["pose"]
        trajectory.write_in_file(fr, out)
    assert text == out.getvalue() and text.count("\n") == len(recs)
    summary = system.report_summary()
    assert summary["keyframes"] == 4 and summary["filters"] == recs[-1]["seeds"]
    assert summary["candidates"] == recs[-1]["candidates"]
    assert system.status == svo_amd.System.PROCESS_NEW_FRAME and system.ref_frame is system.cur_frame


@pytest.mark.gpu
def test_gpu_system_eviction_matches_restatement():
    import svo_amd
    imgs, _ = sequence(9)
    s, want = restatement(2, 9)
    system, recs, _ = gpu_run(imgs, max_keyframes=2)
    compare(recs, want)
    base = system.cur_frame.id - 8
    assert sorted(k.id - base for k in system.map.key_frames) == [4, 7]
    de = system.depth_estimator
    assert all(f.frame.id - base in (4, 7) for f in de.features) and len(de.keyframes) == 2
    assert all(de.keyframes[k] is f.frame for k, f in zip(de.seeds["kf"], de.features))
    for fr in system.map.key_frames + [system.cur_frame]:
        assert all(f.point is None or f.point.type != svo_amd.PointType.DELETED for f in fr.features)


@pytest.mark.gpu
def test_gpu_failure_paths():
    import svo_amd
    imgs, _ = sequence()
    _, want = restatement()
    system = svo_amd.System(svo_amd.Config(**SC.config_kwargs()))
    assert system.add_image(np.full((SC.HEIGHT, SC.WIDTH), 128, np.uint8), 0) is False
    assert system.status == svo_amd.System.PROCESS_FIRST_FRAME and system.ref_frame is None
    assert system.add_image(imgs[0], 1) is True
    first = system.ref_frame
    assert system.add_image(imgs[0], 2) is False                             # no disparity
    assert system.status == svo_amd.System.PROCESS_SECOND_FRAME and system.ref_frame is first
    assert system.add_image(imgs[1], 3) is True
    assert system.status == svo_amd.System.PROCESS_NEW_FRAME and system.map.key_frames[0] is first
    assert system.cur_frame.number_observation() == want[1]["n_obs"]
    assert np.abs(canon(system.cur_frame.abs_pose) - canon(want[1]["pose"])).max() <= POSE_BOUND


@pytest.mark.gpu
def test_gpu_relocalisation_branch():
    """Entered through the setter: one ImageAlignment.align against getClosestKeyframe's frame.  On the eviction
    variant, whose keyframes (4 and 7) both have a last keyframe: the very first keyframe has none, and aligning
    against it dereferences a null m_lastKeyframe in the reference (a ValueError here)."""
    import svo_amd
    imgs, _ = sequence(9)
    system, _, _ = gpu_run(imgs[:8], max_keyframes=2)
    system.set_status(svo_amd.System.PROCESS_RELOCALIZATION)
    assert system.add_image(imgs[8], 8) is True and system.last_result == svo_amd.System.SUCCESS
    cur = system.cur_frame
    c = system.config
    probe = svo_amd.Frame(system.camera, imgs[8], c.max_level_image_pyramid + 1, 8, cur.last_keyframe)
    closest = system.map.get_closest_keyframe(probe)
    assert closest is not None and closest in system.map.key_frames
    # from the identity pose of a new frame every keyframe with a visible point is close; the nearest translation wins
    dists = [(kf, d) for kf, d in system.map.get_close_keyframes(probe)]
    assert closest is min(dists, key=lambda e: e[1])[0]
    svo_amd.ImageAlignment(c.patch_size_image_alignment, c.min_level_image_pyramid, c.max_level_image_pyramid, 6,
                           median_mode=c.median_mode).align(closest, probe)
    assert np.array_equal(probe.abs_pose, cur.abs_pose)
    _, want = restatement(2, 9, True)                                         # and the restatement's branch
    assert np.abs(canon(cur.abs_pose) - canon(want[-1]["pose"])).max() <= POSE_BOUND
    assert system.status == svo_amd.System.PROCESS_RELOCALIZATION and system.ref_frame is cur
    assert system.map.get_furthest_keyframe(probe.camera_in_world()) in system.map.key_frames


# ---------------------------------------------------------------- GPU: the C++ mirror against the Python mirror
def parse_host_system(text):
    """(records, trajectory text, per-frame timings) of one pass of `svo_host_check system`."""
    recs, times, lines = [], [], text.splitlines()
    k = 0
    while lines[k] != "trajectory":
        f = [int(x) for x in lines[k].split()[1:]]
        pose = np.array([float.fromhex(x) for x in lines[k + 1].split()[1:]])
        removed = sorted(tuple(int(v) for v in x.split(":")) for x in lines[k + 2].split()[1:])
        times.append({a: float(b) for a, b in (x.split("=") for x in lines[k + 3].split()[1:])})
        recs.append(dict(result=f[1], status=f[2], keyframe=bool(f[3]), n_obs=f[4], n_obs_points=f[5], seeds=f[6],
                         candidates=f[7], keyframes=f[8], ba_removed=removed, pose=pose))
        k += 4
    return recs, "".join(x + "\n" for x in lines[k + 1:]), times


@pytest.mark.gpu
@pytest.mark.parametrize("max_keyframes,n_frames,relocalise", [(7, 8, False), (2, 9, False), (2, 9, True)])
def test_gpu_cpp_mirror_matches_python_mirror(tmp_path, max_keyframes, n_frames, relocalise):
    """svo_amd::System (build/svo_host_check system) against svo_amd.System on the same frames: both call the same
    ABI with the same arrays, so the discrete fields are equal and the poses equal in every bit (the map's cell order
    is handed over: the C++ mirror's own seeded shuffle is std::mt19937_64's, not numpy's).  The third case enters the
    relocalisation branch at the last frame."""
    import svo_amd
    import svo_amd.synth as synth
    imgs, _ = sequence(n_frames)
    system = svo_amd.System(svo_amd.Config(**SC.config_kwargs(max_keyframes=max_keyframes)), instrument=True)
    base = svo_amd.Frame._frame_counter
    want, text = [], io.StringIO()
    for k, img in enumerate(imgs):
        if relocalise and k == n_frames - 1:
            system.set_status(svo_amd.System.PROCESS_RELOCALIZATION)
        system.add_image(img, k)
        cur = system.cur_frame
        want.append(dict(result=system.last_result, status=system.status, keyframe=cur.is_keyframe(),
                         n_obs=cur.number_observation(), n_obs_points=cur.number_observation_with_points(),
                         seeds=system.depth_estimator.number_filters(), candidates=len(system.map.candidates),
                         keyframes=system.map.size_keyframes(),
                         ba_removed=sorted((f - base, i) for f, i in system.ba_removed),
                         pose=np.array(cur.abs_pose, np.float64)))
        system.write_in_file(text)
    data, raw = synth.write_system_problem(system.config, imgs, system.map.cell_orders, tmp_path, relocalise)
    out = subprocess.run([HOST_CHECK, "system", data, raw], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got, trajectory, _ = parse_host_system(out.stdout)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in EXACT:
            assert g[name] == w[name], (k, name, g[name], w[name])
        assert g["pose"].tobytes() == np.asarray(w["pose"], np.float64).tobytes(), (k, g["pose"], w["pose"])
    assert trajectory == text.getvalue()
    if relocalise:
        assert want[-1]["status"] == svo_amd.System.PROCESS_RELOCALIZATION and want[-1]["result"] == svo_amd.System.SUCCESS
