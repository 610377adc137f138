"""The alignment kernels at every patch size they are built for.

csrc/align.hip builds K1 (align_residual_kernel<kHalf, kWin, kRef>) and K3 (align_weights_kernel<kHalf, kWin>) for
kHalf = 0..9; svo_align_batch_create takes patch_size 1..19 and half = patch_size / 2.  Each half has its own load,
store and staging paths (DESIGN.md §2 has the table), so every patch size 1..19 runs here in both median modes, with
the window hand-over (kWin) forced off (SVO_WIN_LEVELS=0) and on at every level (SVO_WIN_LEVELS=7), against the CPU
oracle in the same median mode at the bounds of tests/test_gpu_parity.py and tests/test_reference_median.py.  The two
window settings read the same image bytes and the build does not contract, so their outputs are bit-equal.

Scenes: 320 x 240, 300 features, levels 0..2.  Every batch holds two pairs with different feature counts (300, and
150 + 70), so that the per-pair slot stride (320 against 256 features) differs from the batch strides and the second
pair's second chunk is empty.  The test ids name the patch, its half and the window setting.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import svo_amd
import svo_amd.synth as synth
from common import canon, check_ref_traces, check_traces, gpu_batch, oracle_align, take
from svo_amd._capi import SvoLevelTrace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "semi-direct-visual-odometry_amd", "csrc", "capi.hip")

W, H, NF, MIN_LEVEL, MAX_LEVEL = 320, 240, 300, 0, 2
PATCHES = list(range(1, 20))
EXACT, REFERENCE = svo_amd.MEDIAN_EXACT, svo_amd.MEDIAN_REFERENCE
ORACLE_MODE = {EXACT: 1, REFERENCE: 0}  # oracle median_mode: 1 exact order statistics, 0 std::nth_element
WIN_OFF, WIN_ON, WIN_RULE = 0, 7, None  # SVO_WIN_LEVELS: no level, levels 0..2, unset (the product's own rule)
LAYC_PATCH = 17                         # take(s, 110, 110): 220 * 289 = 63 580 slots
KSTATUS_NON_SUFF_POINTS, KSTATUS_FAILED = 6, 9

# (n_ref, n_kf) of pair 0 per patch: the pair_active threshold (area 1: 6 slots), single features at areas 9 and 361,
# the 64-feature slot stride and the 256-feature chunk (chunks 1 -> 2), and half 6 (a 4-B load tail) at small counts
EDGES = {1: [(5, 0), (3, 2), (6, 0), (3, 3), (0, 6)],
         2: [(1, 0), (1, 1)],
         13: [(63, 0), (64, 1), (150, 150)],
         19: [(1, 0), (1, 1), (32, 31), (32, 32), (33, 32), (128, 128), (129, 128)]}
INACTIVE = [(5, 0), (3, 2), (0, 6)]  # of patch 1: fewer than 6 residuals, or no ref feature


def area_of(patch):
    return (2 * (patch // 2) + 1) ** 2


@functools.lru_cache(maxsize=None)
def scene(patch, second=False):
    """The full pair of a patch size (never modified: take() copies)."""
    return synth.make_pair(seed=synth.SEED_BASE + (100 if second else 0) + patch, n_features=NF, patch_size=patch,
                           width=W, height=H)


@functools.lru_cache(maxsize=None)
def batch_pairs(patch, kind="full"):
    """kind "full": the 300-feature pair and a 150 + 70 one; "layc": 110 + 110 in front; (n_ref, n_kf): that many
    features in front and about half as many of the same scene behind."""
    if kind == "full":
        return (scene(patch), take(scene(patch, True), 150, 70))
    if kind == "layc":
        return (take(scene(patch), 110, 110), take(scene(patch, True), 150, 70))
    n_ref, n_kf = kind
    return (take(scene(patch), n_ref, n_kf), take(scene(patch), (n_ref + 1) // 2, n_kf // 2))


def pair_is_active(s, patch):  # align() returns early without ref features; optimizeLM needs 6 residuals
    return s.n_ref > 0 and (s.n_ref + s.n_kf) * area_of(patch) >= 6


@functools.lru_cache(maxsize=None)
def oracle_result(patch, kind, i, mode):
    return oracle_align(batch_pairs(patch, kind)[i], patch, MIN_LEVEL, MAX_LEVEL, mode=ORACLE_MODE[mode])


Run = namedtuple("Run", "poses err status traces")
_runs = {}


def device_run(monkeypatch, patch, kind, mode, win):
    """One batch on the GPU, created with SVO_WIN_LEVELS = win (svo_align_batch_create reads it); run once per
    (patch, kind, mode, win) and shared by the tests that compare window settings."""
    key = (patch, kind, mode, win)
    if key not in _runs:
        if win is WIN_RULE:
            monkeypatch.delenv("SVO_WIN_LEVELS", raising=False)
        else:
            monkeypatch.setenv("SVO_WIN_LEVELS", str(win))
        pairs = batch_pairs(patch, kind)
        b, ps = gpu_batch(pairs, patch, MIN_LEVEL, MAX_LEVEL, median_mode=mode)
        b.run()
        poses, err, st = b.results()
        _runs[key] = Run(poses, err, st, [b.traces(i) for i in range(len(pairs))])
        b.close()
        ps.close()
    return _runs[key]


def check_against_oracle(run, patch, kind, mode):
    for i, s in enumerate(batch_pairs(patch, kind)):
        pose_c, err_c, st_c, tr_c = oracle_result(patch, kind, i, mode)
        print(f"patch {patch} {kind} mode {mode} pair {i} ({s.n_ref}+{s.n_kf}): status {run.status[i]} / {st_c}, "
              f"err {run.err[i]!r} / {err_c!r}, pose diff {np.abs(canon(run.poses[i]) - canon(pose_c)).max():.3e}")
        if pair_is_active(s, patch):
            if mode == EXACT:
                check_traces(run.traces[i], tr_c, MIN_LEVEL, MAX_LEVEL, exact_levels={MAX_LEVEL})
            else:
                check_ref_traces(run.traces[i], tr_c, MIN_LEVEL, MAX_LEVEL)
            assert np.abs(canon(run.poses[i]) - canon(pose_c)).max() <= 1e-9, i
            assert abs(run.err[i] - err_c) <= 1e-9 * abs(err_c), i
        else:  # the device leaves such a pair's level traces zeroed (init_pair); the oracle's records differ there
            assert np.array_equal(run.poses[i], s.cur_init_pose) and np.array_equal(pose_c, s.cur_init_pose), i
            assert run.err[i] == err_c == (0.0 if s.n_ref == 0 else -1.0), i
            assert st_c == (KSTATUS_FAILED if s.n_ref == 0 else KSTATUS_NON_SUFF_POINTS), i
        assert run.status[i] == st_c, i


def check_same_bits(run, base, what):
    """Poses, err, status and every trace field of two runs, byte for byte (NaN-safe)."""
    for name in ("poses", "err", "status"):
        a, b = getattr(run, name), getattr(base, name)
        assert a.tobytes() == b.tobytes(), (what, name, a, b)
    diffs = []
    for i, (ta, tb) in enumerate(zip(run.traces, base.traces)):
        for l in range(MAX_LEVEL + 1):
            ra, rb = bytes(ta[l]), bytes(tb[l])
            for name, _ in SvoLevelTrace._fields_:
                f = getattr(SvoLevelTrace, name)
                if ra[f.offset:f.offset + f.size] != rb[f.offset:f.offset + f.size]:
                    va, vb = getattr(ta[l], name), getattr(tb[l], name)
                    diffs.append((i, l, name, list(va) if hasattr(va, "__len__") else va,
                                  list(vb) if hasattr(vb, "__len__") else vb))
    assert not diffs, (what, "(pair, level, field, this run, SVO_WIN_LEVELS=0): the test id of each setting says "
                       "which of the two leaves the oracle", diffs)


def check_batch(monkeypatch, patch, kind, mode, win):
    run = device_run(monkeypatch, patch, kind, mode, win)
    check_against_oracle(run, patch, kind, mode)
    if win != WIN_OFF:
        check_same_bits(run, device_run(monkeypatch, patch, kind, mode, WIN_OFF), (patch, kind, mode, win))


def _win_name(win):
    return {WIN_OFF: "win_off", WIN_ON: "win_on", WIN_RULE: "win_rule"}[win]


def _case(patch, win):
    return pytest.param(patch, win, id=f"patch{patch}-half{patch // 2}-{_win_name(win)}")


# every patch with the hand-over off and on; the product's own rule (the variable unset) at patch 5, where it picks
# level 0 at this size and feature count, and at patch 19, where it picks none
CASES = [_case(p, w) for p in PATCHES for w in (WIN_OFF, WIN_ON)] + [_case(5, WIN_RULE), _case(19, WIN_RULE)]


# ---------------------------------------------------------------- CPU: the scenes and the knob
@pytest.mark.parametrize("patch", PATCHES)
def test_scenes_are_usable(patch):
    """Every pair that the GPU tests align is active and sees slots on every level in both oracle modes: a scene
    that goes blind fails here instead of passing empty there."""
    kinds = ["full"] + (["layc"] if patch == LAYC_PATCH else []) + EDGES.get(patch, [])
    for kind in kinds:
        pairs = batch_pairs(patch, kind)
        if kind == "full":
            assert (len(pairs[0].px), pairs[0].n_ref + pairs[0].n_kf) == (NF, NF)
            assert (pairs[1].n_ref, pairs[1].n_kf, len(pairs[1].px)) == (150, 70, 220)
        for i, s in enumerate(pairs):
            assert len(s.px) == len(s.bearing) == len(s.point) == len(s.has_point) == s.n_ref + s.n_kf
            if i == 0:  # the inactive cases are the intended ones only
                assert pair_is_active(s, patch) == (kind not in INACTIVE), kind
            if not pair_is_active(s, patch):
                continue
            for mode in (EXACT, REFERENCE):
                _, _, st, tr = oracle_result(patch, kind, i, mode)
                assert st == 0, (kind, i, mode, st)
                for l in range(MIN_LEVEL, MAX_LEVEL + 1):
                    assert tr[l].n_vis > 0 and tr[l].n_ref_vis > 0, (kind, i, mode, l)


def test_take_copies_the_leading_features():
    s = scene(5)
    t = take(s, 3, 2)
    assert (t.n_ref, t.n_kf) == (3, 2) and s.n_ref + s.n_kf == NF
    assert np.array_equal(t.px, np.concatenate([s.px[:3], s.px[s.n_ref:s.n_ref + 2]]))
    assert np.array_equal(t.point, np.concatenate([s.point[:3], s.point[s.n_ref:s.n_ref + 2]]))
    t.px[:] = 0.0
    assert s.px[0, 0] != 0.0 and t.ref_img is s.ref_img  # the features are copies, the images shared


def test_slot_counts_cross_the_selection_layouts():
    """300 features put the reference-mode residual vector into each of K2V's layouts and into K2R by the patch size
    alone; the extra patch-17 batch (220 features) lands in LayC.  If the layouts move, this fails instead of the
    GPU tests drifting off the boundaries."""
    laya, layb, layc = svo_amd.SCALE_K2V_LAYA_SLOTS, svo_amd.SCALE_K2V_LAYB_SLOTS, svo_amd.SCALE_K2V_MAX_SLOTS
    slots = {p: NF * area_of(p) for p in PATCHES}
    assert (slots[11], slots[12], slots[13], slots[14]) == (36300, 50700, 50700, 67500)
    assert all(slots[p] <= laya for p in range(1, 12))
    assert all(laya < slots[p] <= layb for p in (12, 13))
    assert all(slots[p] > layc for p in range(14, 20))
    layc_pairs = batch_pairs(LAYC_PATCH, "layc")
    n = max(len(s.px) for s in layc_pairs) * area_of(LAYC_PATCH)  # the batch's largest vector chooses the kernel
    assert n == 63580 and layb < n <= layc


def test_window_knob_is_read_at_batch_creation():
    """SVO_WIN_LEVELS is still read with getenv inside svo_align_batch_create: without the knob the comparison of the
    two window settings would compare a run with itself."""
    src = open(CAPI).read()
    m = re.search(r"^int svo_align_batch_create\(.*?^}", src, re.S | re.M)
    assert m, "svo_align_batch_create not found"
    assert 'getenv("SVO_WIN_LEVELS")' in m.group(0)
    assert re.search(r"win_levels\s*=\s*\(uint32_t\)strtoul\(", m.group(0))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("patch,win", CASES)
def test_align_every_patch_exact(patch, win, monkeypatch):
    check_batch(monkeypatch, patch, "full", EXACT, win)


@pytest.mark.gpu
@pytest.mark.parametrize("patch,win", CASES)
def test_align_every_patch_reference(patch, win, monkeypatch):
    """300 * area slots: K2V LayA up to patch 11, LayB at 12 and 13, K2R from 14 up."""
    check_batch(monkeypatch, patch, "full", REFERENCE, win)


@pytest.mark.gpu
@pytest.mark.parametrize("patch,win", [_case(LAYC_PATCH, WIN_OFF), _case(LAYC_PATCH, WIN_ON)])
def test_align_reference_layc(patch, win, monkeypatch):
    """63 580 slots per pair: K2V's third layout fed by a half-8 K1."""
    check_batch(monkeypatch, patch, "layc", REFERENCE, win)
    run = device_run(monkeypatch, patch, "layc", REFERENCE, win)
    assert all(run.traces[i][l].scale_kernel == svo_amd.SCALE_K2V for i in range(2) for l in range(MAX_LEVEL + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("patch,n_ref,n_kf", [pytest.param(p, a, b, id=f"patch{p}-half{p // 2}-{a}+{b}")
                                              for p, cases in EDGES.items() for (a, b) in cases])
def test_align_feature_count_edges(patch, n_ref, n_kf, monkeypatch):
    for mode in (EXACT, REFERENCE):
        for win in (WIN_OFF, WIN_ON):
            check_batch(monkeypatch, patch, (n_ref, n_kf), mode, win)
