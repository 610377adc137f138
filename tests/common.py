"""Shared helpers for the parity tests: synthetic pairs, oracle runs, GPU batches, per-level trace checks."""
import dataclasses

import numpy as np

import oracle as O
import svo_amd
import svo_amd.synth as synth

KITTI = dict(fx=721.5377, fy=721.5377, cx=609.5593, cy=172.8540, width=1241, height=376)


def canon(p):
    """Quaternion sign canonicalisation (q and -q are the same rotation)."""
    p = np.array(p, dtype=np.float64)
    if p.ndim == 1:
        return p if p[3] >= 0 else np.concatenate([-p[:4], p[4:]])
    s = np.where(p[:, 3:4] >= 0, 1.0, -1.0)
    return np.concatenate([p[:, :4] * s, p[:, 4:]], axis=1)


def make_pairs(n, seed0=synth.SEED_BASE, **kw):
    return [synth.make_pair(seed=seed0 + i, **kw) for i in range(n)]


def take(s, n_ref, n_kf):
    """A copy of pair `s` with its first n_ref ref features and its first n_kf kf features."""
    assert 0 <= n_ref <= s.n_ref and 0 <= n_kf <= s.n_kf, (n_ref, s.n_ref, n_kf, s.n_kf)
    idx = np.concatenate([np.arange(n_ref), s.n_ref + np.arange(n_kf)]).astype(np.int64)
    return dataclasses.replace(s, n_ref=int(n_ref), n_kf=int(n_kf), px=s.px[idx].copy(), bearing=s.bearing[idx].copy(),
                               point=s.point[idx].copy(), has_point=s.has_point[idx].copy())


def oracle_pyramids(s, levels):
    return [O.build_pyramid(im, levels)[0] for im in (s.ref_img, s.kf_img, s.cur_img)]


def oracle_align(s, patch, min_level, max_level, mode=0, trace=True, init=None):
    pyr = oracle_pyramids(s, max_level + 1)
    pair = O.make_pair(pyr[0], pyr[1], pyr[2], s.ref_pose, s.kf_pose, s.n_ref, s.n_kf, s.px, s.bearing, s.point,
                       s.has_point)
    return O.image_align(s.camera, patch, min_level, max_level, pair,
                         s.cur_init_pose if init is None else init, median_mode=mode, trace=trace)


def gpu_batch(pairs, patch, min_level, max_level, ctx=None, max_features=None, median_mode=svo_amd.MEDIAN_EXACT):
    """Upload every pair (3 frames each) into one PyramidSet and one AlignBatch; returns (batch, set)."""
    cam = pairs[0].camera
    camera = svo_amd.PinholeCamera(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ps = svo_amd.PyramidSet(3 * len(pairs), cam["width"], cam["height"], max_level + 1, ctx)
    imgs = np.stack([im for s in pairs for im in (s.ref_img, s.kf_img, s.cur_img)])
    ps.upload(0, imgs)
    ps.build()
    mf = max_features or max(max(len(s.px) for s in pairs), 1)
    b = svo_amd.AlignBatch(camera, patch, min_level, max_level, len(pairs), mf, ctx, median_mode=median_mode)
    for i, s in enumerate(pairs):
        b.set_pair(i, (ps, 3 * i), (ps, 3 * i + 1), (ps, 3 * i + 2), s.ref_pose, s.kf_pose, s.cur_init_pose,
                   s.n_ref, s.n_kf, s.px, s.bearing, s.point, s.has_point)
    return b, ps


def check_traces(tr_gpu, tr_cpu, min_level, max_level, exact_levels):
    """Per-level traces of an exact-mode alignment against the oracle's (median_mode 1): DESIGN.md §2."""
    for l in range(max_level, min_level - 1, -1):
        g, c = tr_gpu[l], tr_cpu[l]
        assert (g.n_ref_vis, g.n_vis, g.status) == (c.n_ref_vis, c.n_vis, c.status), (l, g.n_vis, c.n_vis)
        if l in exact_levels:
            assert g.median == c.median and g.mad == c.mad and g.sigma == c.sigma, l
        else:
            assert abs(g.sigma - c.sigma) <= 1e-9 * abs(c.sigma), l
        Hg = np.tril(np.array(g.H).reshape(6, 6))
        Hc = np.tril(np.array(c.H).reshape(6, 6))
        assert np.abs(Hg - Hc).max() <= 1e-10 * np.abs(Hc).max(), l
        gg, gc = np.array(g.g), np.array(c.g)
        assert np.abs(gg - gc).max() <= 1e-9 * max(np.abs(gc).max(), 1e-300), l
        assert abs(g.chi2 - c.chi2) <= 1e-10 * c.chi2, l


def check_ref_traces(tr_gpu, tr_cpu, min_level, max_level):
    """Per-level traces of a reference-mode alignment against the oracle's std::nth_element path (median_mode 0)."""
    for l in range(max_level, min_level - 1, -1):
        g, c = tr_gpu[l], tr_cpu[l]
        assert (g.n_ref_vis, g.n_vis, g.status) == (c.n_ref_vis, c.n_vis, c.status), (l, g.n_vis, c.n_vis)
        if l == max_level:  # later levels start from poses that differ by ~1e-13 (summation order)
            assert (g.median, g.mad, g.sigma) == (c.median, c.mad, c.sigma), (l, g.median, c.median, g.mad, c.mad)
        else:
            assert abs(g.sigma - c.sigma) <= 1e-9 * abs(c.sigma), l
