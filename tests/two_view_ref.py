"""numpy restatement of the two-view map initialisation (src/system.cpp:144-223 with src/algorithm.cpp:173-333,
:553-599, :655-680, :813-832) and the synthetic scenes tests/test_two_view_init.py runs it on.

The restatement is float64 numpy written independently of the product's code: numpy.linalg.svd for the essential
matrix, matrix-form poses, a vectorised unpivoted elimination for the 3x3 normal equations.  `dtype` switches the
per-match part (triangulation, camera points, depths, rescaling) to numpy.longdouble for the extended-precision
comparison that fixes the points' tolerance.
"""
import os
import subprocess

import numpy as np

from common import KITTI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
W_MAT = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # src/algorithm.cpp:246
# relabelings of (R1,t) (R1,-t) (R2,t) (R2,-t) that another valid SVD of the same E can produce: t <-> -t, R1 <-> R2
RELABELINGS = [(0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0)]


def K_of(cam=KITTI):
    return np.array([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])


def invK_of(cam=KITTI):  # src/pinhole_camera.cpp:24
    return np.array([[1 / cam["fx"], 0.0, -cam["cx"] / cam["fx"]], [0.0, 1 / cam["fy"], -cam["cy"] / cam["fy"]],
                     [0.0, 0.0, 1.0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = skew(k)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def quat_to_R(q):  # (x, y, z, w)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_quat()


def pose_to_Rt(p):
    p = np.asarray(p, np.float64)
    return quat_to_R(p[:4]), p[4:7].copy()


def Rt_to_pose(R, t):
    return np.concatenate([R_to_quat(R), t])


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


class Scene:
    pass


def make_scene(seed, n, kind="side", noise=0.3, ref_pose=None, baseline=0.5, cam=KITTI):
    """n matches of a frame pair: reference pixels uniform at least 20 px inside the frame, depths 6-60, a small
    rotation plus a sideways-dominant (or forward) translation, current pixels = projection + N(0, noise) px,
    E = [t^]x R for the relative motion X_cur = R X_ref + t."""
    rng = np.random.default_rng(seed)
    K, iK = K_of(cam), invK_of(cam)
    s = Scene()
    s.n, s.kind, s.seed = n, kind, seed
    s.ref_pose = IDENTITY.copy() if ref_pose is None else np.asarray(ref_pose, np.float64)
    u = np.stack([rng.uniform(20.0, cam["width"] - 20.0, n), rng.uniform(20.0, cam["height"] - 20.0, n)], axis=1)
    depth = rng.uniform(6.0, 60.0, n)
    Xr = (iK @ np.concatenate([u, np.ones((n, 1))], axis=1).T).T * depth[:, None]
    R = rodrigues(rng.normal(size=3) * 0.01)
    d = np.array([1.0, 0.05, 0.1]) if kind == "side" else np.array([0.02, 0.01, 1.0])
    t = baseline * d / np.linalg.norm(d)
    Xc = Xr @ R.T + t
    v = (K @ Xc.T).T
    v = v[:, :2] / v[:, 2:3]
    s.ref_px = np.ascontiguousarray(u)
    s.cur_px = np.ascontiguousarray(v + rng.normal(size=(n, 2)) * noise)
    s.R_true, s.t_true, s.depth_true, s.X_ref_true = R, t, depth, Xr
    s.E = skew(t / np.linalg.norm(t)) @ R
    return s


# ------------------------------------------------------------------ the restatement
def fundamental(E, cam=KITTI):
    iK = invK_of(cam)
    T = np.zeros((3, 3))
    F = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            T[i, j] = iK[0, i] * E[0, j] + iK[1, i] * E[1, j] + iK[2, i] * E[2, j]
    for i in range(3):
        for j in range(3):
            F[i, j] = T[i, 0] * iK[0, j] + T[i, 1] * iK[1, j] + T[i, 2] * iK[2, j]
    return F


def fundamental_bound(E, cam=KITTI):
    """|invK^T| |E| |invK|: the scale of each entry's rounding error (two 3x3 products)."""
    iK = np.abs(invK_of(cam))
    return iK.T @ np.abs(E) @ iK


def sampson(F, ref_px, cur_px):
    """algorithm::sampsonCorrection (src/algorithm.cpp:196-235): the same IEEE operations in the same order (numpy
    evaluates each * and + as one rounded operation), so the result is the reference's bit for bit."""
    x0x, x0y, x1x, x1y = ref_px[:, 0], ref_px[:, 1], cur_px[:, 0], cur_px[:, 1]
    upper = (x0x * ((x1x * F[0, 0]) + (x1y * F[1, 0]) + F[2, 0])) + \
            (x0y * ((x1x * F[0, 1]) + (x1y * F[1, 1]) + F[2, 1])) + (x1x * F[0, 2]) + (x1y * F[1, 2]) + F[2, 2]
    t0 = ((F[0, 0] * x0x) + (F[0, 1] * x0y) + F[0, 2])
    t1 = ((F[1, 0] * x0x) + (F[1, 1] * x0y) + F[1, 2])
    t2 = ((F[0, 0] * x1x) + (F[1, 0] * x1y) + F[2, 0])
    t3 = ((F[0, 1] * x1x) + (F[1, 1] * x1y) + F[2, 1])
    lower = ((t0 * t0) + (t1 * t1) + (t2 * t2) + (t3 * t3))
    f = upper / lower
    return (np.stack([x0x - (f * t2), x0y - (f * t3)], axis=1), np.stack([x1x - (f * t0), x1y - (f * t1)], axis=1))


def hypotheses(E):
    """decomposeEssentialMatrix + the four poses of recoverPose (src/algorithm.cpp:241-286) as (R, t) pairs.  The
    rotations are re-orthogonalised by projecting on SO(3) (the reference's angle-axis round trip changes an
    orthogonal matrix by rounding only)."""
    U, _, Vt = np.linalg.svd(E)
    out = []
    t = U[:, 2]
    for Wm in (W_MAT, W_MAT.T):
        R = U @ Wm @ Vt
        if np.linalg.det(R) < 0:
            R = -R
        u, _, vt = np.linalg.svd(R)
        R = u @ vt
        out += [(R, t.copy()), (R, -t)]
    return out


def _solve3(H, g):
    """x of H x = g for stacks of symmetric positive 3x3 (n, 3, 3), (n, 3): elimination without pivoting, any dtype."""
    a, b, c = H[:, 0, 0], H[:, 1, 0], H[:, 2, 0]
    d, e, f = H[:, 1, 1], H[:, 2, 1], H[:, 2, 2]
    l10, l20 = b / a, c / a
    d1 = d - l10 * b
    e1 = e - l20 * b
    l21 = e1 / d1
    f1 = f - l20 * c - l21 * e1
    y0 = g[:, 0]
    y1 = g[:, 1] - l10 * y0
    y2 = g[:, 2] - l20 * y0 - l21 * y1
    x2 = y2 / f1
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / a - l10 * x1 - l20 * x2
    return np.stack([x0, x1, x2], axis=1)


def triangulate(K, R1, t1, R2, t2, ref_px, cur_px, dtype=np.float64, want_cond=False):
    """algorithm::triangulatePointDLT (src/algorithm.cpp:655-680) for every match."""
    P1 = (K @ np.concatenate([R1, t1[:, None]], axis=1)).astype(dtype)
    P2 = (K @ np.concatenate([R2, t2[:, None]], axis=1)).astype(dtype)
    rp, cp = ref_px.astype(dtype), cur_px.astype(dtype)
    A = np.stack([P1[0, :3] - rp[:, 0:1] * P1[2, :3], P1[1, :3] - rp[:, 1:2] * P1[2, :3],
                  P2[0, :3] - cp[:, 0:1] * P2[2, :3], P2[1, :3] - cp[:, 1:2] * P2[2, :3]], axis=1)  # (n, 4, 3)
    p = np.stack([rp[:, 0] * P1[2, 3] - P1[0, 3], rp[:, 1] * P1[2, 3] - P1[1, 3],
                  cp[:, 0] * P2[2, 3] - P2[0, 3], cp[:, 1] * P2[2, 3] - P2[1, 3]], axis=1)           # (n, 4)
    H = np.einsum("nki,nkj->nij", A, A)
    g = np.einsum("nki,nk->ni", A, p)
    X = _solve3(H, g)
    if want_cond:
        return X, np.linalg.cond(H.astype(np.float64)) if len(H) else np.zeros(0)
    return X


def order_statistic_median(v):
    s = np.sort(v)
    mid = len(s) // 2
    return s[mid] if len(s) % 2 else (s[mid - 1] + s[mid]) / 2.0


_median_exe = None


def median_tool(tmp_dir):
    """Build tests/cpp/median_check.cpp (algorithm::computeMedian with the real std::nth_element) once."""
    global _median_exe
    if _median_exe is None:
        exe = os.path.join(str(tmp_dir), "median_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "median_check.cpp")],
                       check=True)
        _median_exe = exe
    return _median_exe


def reference_median(v, tmp_dir):
    """computeMedian(const VectorXd&) of v: (lo, hi, median) with lo = vec[mid-1], hi = vec[mid] as the reference
    reads them (odd length: lo = hi = the order statistic, from numpy; even: from the real std::nth_element)."""
    v = np.ascontiguousarray(v, np.float64)
    if len(v) % 2:
        m = float(np.sort(v)[len(v) // 2])
        return m, m, m
    path = os.path.join(str(tmp_dir), f"median_{os.getpid()}_{len(v)}.bin")
    v.tofile(path)
    out = subprocess.run([median_tool(tmp_dir), path], capture_output=True, text=True, check=True, timeout=60).stdout
    lo, hi, med = (float.fromhex(x) for x in out.split())
    return lo, hi, med


class Result:
    pass


def two_view_init(E, ref_pose, ref_px, cur_px, map_scale, cell_size, tmp_dir, F=None, cam=KITTI, dtype=np.float64):
    """The whole path for one pair.  F: evaluate the Sampson correction with this matrix (the one the product
    returned) instead of the restatement's own."""
    r = Result()
    K = K_of(cam)
    n = len(ref_px)
    r.F = fundamental(E, cam)
    r.ref_px, r.cur_px = sampson(r.F if F is None else F, ref_px, cur_px)
    Rr, tr = pose_to_Rt(ref_pose)
    r.hyp = hypotheses(E)
    r.counts = np.zeros(4, np.int64)
    r.borderline = np.zeros(n, bool)
    for h, (Rh, th) in enumerate(r.hyp):
        Rc, tc = Rh @ Rr, Rh @ tr + th  # poses[i] * refFrame->m_absPose (src/algorithm.cpp:297)
        X = triangulate(K, Rr, tr, Rc, tc, r.ref_px, r.cur_px)
        zr = (X @ Rr.T + tr)[:, 2]
        zc = (X @ Rc.T + tc)[:, 2]
        nx = np.linalg.norm(X, axis=1)
        r.borderline |= (np.abs(zr) < 1e-9 * nx) | (np.abs(zc) < 1e-9 * nx)
        r.counts[h] = int(np.count_nonzero((zr > 0) & (zc > 0)))
    r.winner = -1
    best = 0
    for h in range(4):
        if r.counts[h] > best:  # the first strictly largest (:318)
            best, r.winner = int(r.counts[h]), h
    r.unique_winner = int(np.count_nonzero(r.counts == best)) == 1
    r.valid = np.zeros(n, np.uint8)
    r.survivor = np.full(n, -1, np.int32)
    r.n_valid = 0
    r.median_depth = float("nan")
    if r.winner < 0:
        return r
    Rw, tw = r.hyp[r.winner]  # poses[winner] alone (:329)
    X, r.cond = triangulate(K, Rr, tr, Rw, tw, r.ref_px, r.cur_px, dtype, want_cond=True)
    Rwd, twd = Rw.astype(dtype), tw.astype(dtype)
    pc = X @ Rwd.T + twd
    r.depth = np.sqrt((pc * pc).sum(axis=1))
    d64 = r.depth.astype(np.float64)
    lo, hi, med = reference_median(d64, tmp_dir)
    r.median_depth = med
    # the same two elements in the working precision
    ilo, ihi = int(np.nonzero(d64 == lo)[0][0]), int(np.nonzero(d64 == hi)[0][0])
    med_w = (r.depth[ilo] + r.depth[ihi]) / dtype(2)
    r.median_index = (ilo, ihi)
    scale = dtype(map_scale) / med_w
    Cr = -(Rr.T @ tr)
    Cc = (-(Rwd.T @ twd))
    C = Cr.astype(dtype) + scale * (Cc - Cr.astype(dtype))
    tn = -(Rwd @ C)  # src/system.cpp:184-186
    r.cur_R, r.cur_t = Rw, tn.astype(np.float64)
    pcs = pc * scale
    r.points_world = (pcs - tn) @ Rwd  # R^T (p - t)
    r.points_cur_scaled = pcs
    hb = float(np.ceil(cell_size / 2.0))
    W, H = cam["width"], cam["height"]

    def inside(p):
        return (p[:, 0] >= hb) & (p[:, 1] >= hb) & (p[:, 0] < W - hb) & (p[:, 1] < H - hb)

    def edge(p):  # within 1e-9 px of an isInFrame threshold
        return (np.abs(p[:, 0] - hb) < 1e-9) | (np.abs(p[:, 1] - hb) < 1e-9) | \
               (np.abs(p[:, 0] - (W - hb)) < 1e-9) | (np.abs(p[:, 1] - (H - hb)) < 1e-9)

    r.valid = (inside(r.ref_px) & inside(r.cur_px) & (pcs[:, 2] > 0)).astype(np.uint8)
    r.borderline |= edge(r.ref_px) | edge(r.cur_px) | \
        (np.abs(pcs[:, 2].astype(np.float64)) < 1e-9 * np.linalg.norm(r.points_world.astype(np.float64), axis=1))
    idx = np.nonzero(r.valid)[0]
    r.n_valid = len(idx)
    r.survivor[:len(idx)] = idx
    return r
