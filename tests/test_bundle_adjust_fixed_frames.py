"""svo_bundle_adjust with more frames than SVO_BA_MAX_FRAMES: the limit counts the free frames only.

localBA holds every observing frame outside the keyframe list as a fixed frame, and a point keeps the observers of
every frame that ever saw it, so the tracker (System, tests/test_system.py) reaches 17 frames in one problem after
sixteen images.  A fixed frame only contributes its constant transform to the edges it observes; nothing of it enters
the reduced system, so their number is unlimited now.

The checker and the bounds are those of tests/test_bundle_adjust.py: the numpy restatement of the contract and 8 * T
per output kind.  T was measured there over scenes of which the ones with fixed frames (which remove the gauge
freedom, as here) measure 1e-15 to 1e-12, so the bound is not widened for this scene."""
import numpy as np
import pytest

import bundle_adjust_ref as B
from test_bundle_adjust import C_GPU, T_CHI, T_CHI2, T_POINT, T_ROT, T_TRANS, _c_call, differences, sequence


def wide_scene():
    """40 frames, the first 30 fixed, 10 free; 150 points with 2..12 observers each, 5 % outliers."""
    return B.Scene(311, 40, 30, 150, 2, 12, outliers=0.05, structure_iterations=10)


def test_layout_checks_count_free_frames():
    s = wide_scene()
    r, msg = _c_call(s)  # 40 frames, 10 free: the layout passes, the null context is what fails
    assert r != 0 and "ctx" in msg, msg
    fixed = s.fixed.copy()
    fixed[:23] = 1
    fixed[23:] = 0      # 17 free
    r, msg = _c_call(s, fixed=fixed)
    assert r != 0 and "17 frames" in msg, msg
    # a duplicate (frame, point) in a frame past 32 is still caught
    o = int(np.nonzero(s.obs_frame >= 33)[0][0])
    of, op = s.obs_frame.copy(), s.obs_point.copy()
    j = op[o]
    k = int(np.nonzero(op == j)[0][0])
    if k == o:
        k += 1
    of[k] = of[o]
    r, msg = _c_call(s, of=of, op=op)
    assert r != 0 and "duplicate" in msg, msg


@pytest.mark.gpu
def test_gpu_forty_frames_thirty_fixed_match_restatement():
    import svo_amd
    s = wide_scene()
    want = s.run()
    poses, points = s.poses.copy(), s.points.copy()
    r = svo_amd.bundle_adjust_batch(svo_amd.PinholeCamera.kitti(), [0, 40], [0, len(points)], [0, len(s.obs_frame)],
                                    poses, s.fixed, points, s.obs_frame, s.obs_point, s.obs_px, s.delta, 10, 10, True)
    got = dict(poses=poses, points=points, obs_chi2=r.obs_chi2, init_chi=r.init_chi[0], final_chi=r.final_chi[0])
    assert r.status[0] == want["status"] and r.iterations[0] == want["iterations"]
    assert sequence([t for t in r.trace[0] if t[0] >= 0]) == sequence(want["trace"])
    assert np.array_equal(poses[:30], s.poses[:30])      # fixed frames are not written
    assert not np.array_equal(poses[30:], s.poses[30:])
    d = differences(got, want)
    print(d)
    assert d["rot"] <= C_GPU * T_ROT and d["trans"] <= C_GPU * T_TRANS and d["point"] <= C_GPU * T_POINT
    assert d["chi2"] <= C_GPU * T_CHI2 and d["chi"] <= C_GPU * T_CHI
    assert want["final_chi"] < want["init_chi"] and want["iterations"] > 0  # (the outliers keep the Huber cost up)


@pytest.mark.gpu
def test_gpu_tracker_runs_past_sixteen_frames():
    """Twenty images through svo_amd.System: at frame 16 localBA has 7 keyframes and 10 fixed observers.  A smoke
    test of the lifted limit only: a 20-frame sequence cuts wider textures, hence other images than the 8- and 9-frame
    ones, and no restatement stands behind this run; it asserts that nothing failed and what the map holds."""
    import svo_amd
    import system_scene as SC
    imgs, _ = SC.make_sequence(20)
    system = svo_amd.System(svo_amd.Config(**SC.config_kwargs()))
    results = [system.add_image(img, k) for k, img in enumerate(imgs)]
    assert all(results) and system.map.size_keyframes() == 7
    frames = {id(f.frame) for kf in system.map.key_frames for g in kf.features if g.point is not None
              for f in g.point.features}
    assert len(frames) > svo_amd.BA_MAX_FRAMES
