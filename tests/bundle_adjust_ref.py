"""numpy restatement of the windowed bundle adjustment contract (include/svo_c.h, svo_bundle_adjust), the checker of
tests/test_bundle_adjust.py, and the synthetic scenes those tests share.

The contract is this project's own, modelled on g2o's OptimizationAlgorithmLevenberg with EdgeProjectXYZ2UV edges as
BundleAdjustment::twoViewBA / localBA set them up (src/bundle_adjustment.cpp:304-339, :397-625).  It is NOT pinned to
g2o: g2o is not part of the reference tree, so nothing here was compared with its bits.

Everything runs in the dtype it is given (float64 or numpy.longdouble): the 3x3 inverses, the Schur complement and
the Cholesky factorisation of the reduced system are written out here instead of taken from LAPACK, which has no
longdouble.  Sums over observations run in observation order (numpy.add.at is sequential), so reversing the
observation arrays reverses every such sum."""
import functools

import numpy as np

from common import KITTI

FAIL_LIMIT = 5


# ---------------------------------------------------------------- SE(3) as csrc/svo_math.h has it
def rotmat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0] = 1 - (tyy + tzz); R[..., 0, 1] = txy - twz; R[..., 0, 2] = txz + twy
    R[..., 1, 0] = txy + twz; R[..., 1, 1] = 1 - (txx + tzz); R[..., 1, 2] = tyz - twx
    R[..., 2, 0] = txz - twy; R[..., 2, 1] = tyz + twx; R[..., 2, 2] = 1 - (txx + tyy)
    return R


def hat(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def se3_exp(a):
    """(upsilon; omega) -> (qx, qy, qz, qw, tx, ty, tz), Sophus with epsilon 1e-10."""
    dt = a.dtype.type
    up, om = a[:3], a[3:]
    theta_sq = om @ om
    if theta_sq < 1e-20:
        theta = dt(0)
        imag = dt(0.5) - dt(1) / 48 * theta_sq + dt(1) / 3840 * theta_sq * theta_sq
        real = dt(1) - dt(1) / 8 * theta_sq + dt(1) / 384 * theta_sq * theta_sq
    else:
        theta = np.sqrt(theta_sq)
        imag = np.sin(theta / 2) / theta
        real = np.cos(theta / 2)
    q = np.array([imag * om[0], imag * om[1], imag * om[2], real], a.dtype)
    W = hat(om)
    if theta < 1e-10:
        V = rotmat(q)
    else:
        V = np.eye(3, dtype=a.dtype) + (1 - np.cos(theta)) / theta_sq * W + (theta - np.sin(theta)) / (theta_sq * theta) * (W @ W)
    return np.concatenate([q, V @ up])


def qmul(a, b):
    r = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                  a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                  a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], a.dtype)
    n2 = r @ r
    if n2 != 1:
        r = r * (2 / (1 + n2))
    return r


def se3_compose(a, b):
    return np.concatenate([qmul(a[:4], b[:4]), a[4:] + rotmat(a[:4]) @ b[4:]])


# ---------------------------------------------------------------- the contract
def edges(R, t, X, of, op, px, f, cx, cy, delta):
    """c, e, e2, w, rho of every edge."""
    c = np.einsum("mij,mj->mi", R[of], X[op]) + t[of]
    e = np.stack([px[:, 0] - (f * c[:, 0] / c[:, 2] + cx), px[:, 1] - (f * c[:, 1] / c[:, 2] + cy)], 1)
    e2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    s = np.sqrt(e2)
    big = s > delta
    rho = np.where(big, 2 * delta * s - delta * delta, e2)
    w = np.where(big, delta / np.where(big, s, 1), 1).astype(e2.dtype)
    return c, e, e2, w, rho


def jacobians(R, of, c, f):
    """J_p = A [I | -hat(c)] (M, 2, 6) and J_x = A R (M, 2, 3), A = d proj / d c."""
    M = len(of)
    iz = 1 / c[:, 2]
    A = np.zeros((M, 2, 3), c.dtype)
    A[:, 0, 0] = f * iz
    A[:, 1, 1] = f * iz
    A[:, 0, 2] = -(f * c[:, 0]) * iz * iz
    A[:, 1, 2] = -(f * c[:, 1]) * iz * iz
    D = np.zeros((M, 3, 6), c.dtype)
    D[:, 0, 0] = D[:, 1, 1] = D[:, 2, 2] = 1
    D[:, 0, 4] = c[:, 2]; D[:, 0, 5] = -c[:, 1]
    D[:, 1, 3] = -c[:, 2]; D[:, 1, 5] = c[:, 0]
    D[:, 2, 3] = c[:, 1]; D[:, 2, 4] = -c[:, 0]
    return A @ D, A @ R[of]


def sym3_inverse(V, lam):
    """(V + lam I)^-1 of a stack of symmetric 3x3 through the Cholesky factor; ok False at a non-positive pivot."""
    with np.errstate(all="ignore"):
        a = V[:, 0, 0] + lam
        l00 = np.sqrt(a); l10 = V[:, 1, 0] / l00; l20 = V[:, 2, 0] / l00
        d1 = (V[:, 1, 1] + lam) - l10 * l10
        l11 = np.sqrt(d1); l21 = (V[:, 2, 1] - l20 * l10) / l11
        d2 = ((V[:, 2, 2] + lam) - l20 * l20) - l21 * l21
        l22 = np.sqrt(d2)
        ok = (a > 0) & (d1 > 0) & (d2 > 0)
        m00, m11, m22 = 1 / l00, 1 / l11, 1 / l22
        m10 = -(l10 * m00) / l11
        m20 = -(l20 * m00 + l21 * m10) / l22
        m21 = -(l21 * m11) / l22
        Vi = np.empty_like(V)
        Vi[:, 0, 0] = m00 * m00 + m10 * m10 + m20 * m20
        Vi[:, 0, 1] = Vi[:, 1, 0] = m10 * m11 + m20 * m21
        Vi[:, 0, 2] = Vi[:, 2, 0] = m20 * m22
        Vi[:, 1, 1] = m11 * m11 + m21 * m21
        Vi[:, 1, 2] = Vi[:, 2, 1] = m21 * m22
        Vi[:, 2, 2] = m22 * m22
    return Vi, ok


def cholesky_solve(S, rhs):
    """x with S x = rhs by a plain Cholesky (any float dtype), or None at a non-positive pivot."""
    n = len(rhs)
    L = np.zeros_like(S)
    for k in range(n):
        d = S[k, k] - L[k, :k] @ L[k, :k]
        if not d > 0:
            return None
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = (S[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    y = np.zeros_like(rhs)
    for k in range(n):
        y[k] = (rhs[k] - L[k, :k] @ y[:k]) / L[k, k]
    x = np.zeros_like(rhs)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - L[k + 1:, k] @ x[k + 1:]) / L[k, k]
    return x


def lambda_factor(r):
    return np.maximum(1 / 3, np.minimum(1 - (2 * r - 1) ** 3, 2 / 3))


def structure_only(R, t, X, of, op, px, f, cx, cy, delta, iterations):
    """Every point on its own with all poses held: the schedule on its 3x3 system, its own lambda and nu."""
    P = len(X)
    dt = X.dtype
    X = X.copy()
    lam = np.zeros(P, dt)
    nu = np.full(P, 2, dt)
    active = np.ones(P, bool)

    def per_point(v):
        out = np.zeros((P,) + v.shape[1:], dt)
        np.add.at(out, op, v)
        return out

    for it in range(iterations):
        c, e, _, w, rho = edges(R, t, X, of, op, px, f, cx, cy, delta)
        _, Jx = jacobians(R, of, c, f)
        cur = per_point(rho)
        V = per_point(np.einsum("m,mki,mkj->mij", w, Jx, Jx))
        g = per_point(np.einsum("m,mki,mk->mi", w, Jx, e))
        if it == 0:
            lam = 1e-5 * np.maximum(V[:, 0, 0], np.maximum(V[:, 1, 1], V[:, 2, 2]))
        pending = active.copy()
        for _q in range(FAIL_LIMIT):
            Vi, ok = sym3_inverse(V, lam)
            with np.errstate(all="ignore"):
                d = np.einsum("pij,pj->pi", Vi, g)
                Xn = X + d
                tmp = per_point(edges(R, t, Xn, of, op, px, f, cx, cy, delta)[4])
                scale = np.einsum("pi,pi->p", d, lam[:, None] * d + g) + 1e-3
                r = (cur - tmp) / scale
                acc = pending & ok & np.isfinite(tmp) & (r > 0)
            X[acc] = Xn[acc]
            lam[acc] = lam[acc] * lambda_factor(r[acc])
            nu[acc] = 2
            rej = pending & ~acc
            lam[rej] = lam[rej] * nu[rej]
            nu[rej] = nu[rej] * 2
            pending = rej
            if not pending.any():
                break
        active &= ~pending
    return X


def bundle_adjust(cam, poses, fixed, points, obs_frame, obs_point, obs_px, delta, max_iterations=10,
                  structure_iterations=0, dtype=np.float64):
    """One problem.  Returns a dict: poses, points, obs_chi2, init_chi, final_chi, iterations, status and trace, a list
    of (iteration, trial, accepted, lambda, r, chi).  The observations need not be grouped here."""
    dt = np.dtype(dtype).type
    f, cx, cy = dt(cam["fx"]), dt(cam["cx"]), dt(cam["cy"])  # fx on both axes
    delta = dt(delta)
    poses = np.array(poses, dtype).reshape(-1, 7)
    X = np.array(points, dtype).reshape(-1, 3)
    px = np.array(obs_px, dtype).reshape(-1, 2)
    of = np.asarray(obs_frame, np.int64)
    op = np.asarray(obs_point, np.int64)
    fixed = np.asarray(fixed, bool)
    F, P, M = len(poses), len(X), len(of)
    out = dict(poses=poses, points=X, obs_chi2=np.zeros(M, dtype), init_chi=dt(0), final_chi=dt(0), iterations=0,
               status=-1, trace=[])
    if P == 0 or F == 0:
        return out
    ridx = np.full(F, -1)
    ridx[~fixed] = np.arange((~fixed).sum())
    nfree = int((~fixed).sum())
    n = 6 * nfree
    fo = np.nonzero(ridx[of] >= 0)[0]          # the edges on free frames, in observation order
    rf = ridx[of[fo]]
    # ordered pairs of free edges of one point (both orders and each edge with itself), in observation order
    pa, pb = [], []
    by_point = {}
    for k, o in enumerate(fo):
        by_point.setdefault(op[o], []).append(k)
    for ks in by_point.values():
        for ka in ks:
            for kb in ks:
                pa.append(ka)
                pb.append(kb)
    pa, pb = np.array(pa, np.int64), np.array(pb, np.int64)

    def geometry(poses):
        return rotmat(poses[:, :4]), poses[:, 4:]

    R, t = geometry(poses)
    if structure_iterations > 0:
        X = structure_only(R, t, X, of, op, px, f, cx, cy, delta, structure_iterations)
    cur = edges(R, t, X, of, op, px, f, cx, cy, delta)[4].sum()
    out["init_chi"] = cur
    lam, nu = dt(0), dt(2)
    iters, status = 0, 0
    for it in range(max_iterations):
        c, e, _, w, _ = edges(R, t, X, of, op, px, f, cx, cy, delta)
        Jp, Jx = jacobians(R, of, c, f)
        V = np.zeros((P, 3, 3), dtype)
        np.add.at(V, op, np.einsum("m,mki,mkj->mij", w, Jx, Jx))
        g = np.zeros((P, 3), dtype)
        np.add.at(g, op, np.einsum("m,mki,mk->mi", w, Jx, e))
        U = np.zeros((nfree, 6, 6), dtype)
        np.add.at(U, rf, np.einsum("m,mki,mkj->mij", w[fo], Jp[fo], Jp[fo]))
        b = np.zeros((nfree, 6), dtype)
        np.add.at(b, rf, np.einsum("m,mki,mk->mi", w[fo], Jp[fo], e[fo]))
        W = np.einsum("m,mki,mkj->mij", w[fo], Jp[fo], Jx[fo])  # (free edges, 6, 3)
        if it == 0:
            diag = [V[:, k, k].max() for k in range(3)] + [U[:, k, k].max() for k in range(6) if nfree]
            lam = 1e-5 * max(diag)
        accepted = False
        for q in range(FAIL_LIMIT):
            Vi, okv = sym3_inverse(V, lam)
            dx = None
            if okv.all():
                Y = W @ Vi[op[fo]]
                S4 = np.zeros((nfree, nfree, 6, 6), dtype)
                for k in range(nfree):
                    S4[k, k] = U[k] + lam * np.eye(6, dtype=dtype)
                if len(pa):
                    np.subtract.at(S4, (rf[pa], rf[pb]), np.einsum("kim,kjm->kij", Y[pa], W[pb]))
                S = S4.transpose(0, 2, 1, 3).reshape(n, n)
                rhs = b.copy()
                np.subtract.at(rhs, rf, np.einsum("kim,km->ki", Y, g[op[fo]]))
                dp = cholesky_solve(S, rhs.reshape(n)) if n else np.zeros(0, dtype)
                if dp is not None:
                    h = g.copy()
                    np.subtract.at(h, op[fo], np.einsum("kim,ki->km", W, dp.reshape(nfree, 6)[rf]))
                    dx = np.einsum("pij,pj->pi", Vi, h)
            r, tmp, acc = dt(0), cur, False
            if dx is not None:
                trial = poses.copy()
                for i in range(F):
                    if ridx[i] >= 0:
                        trial[i] = se3_compose(se3_exp(dp[6 * ridx[i]:6 * ridx[i] + 6]), poses[i])
                Rt, tt = geometry(trial)
                Xt = X + dx
                with np.errstate(all="ignore"):
                    tmp = edges(Rt, tt, Xt, of, op, px, f, cx, cy, delta)[4].sum()
                    scale = dp @ (lam * dp + b.reshape(n)) + np.einsum("pi,pi->", dx, lam * dx + g) + 1e-3
                    r = (cur - tmp) / scale
                acc = bool(r > 0 and np.isfinite(tmp))
            out["trace"].append((it, q, int(acc), lam, r, tmp))
            if acc:
                poses, X, R, t, cur = trial, Xt, Rt, tt, tmp
                lam = lam * lambda_factor(r)
                nu = dt(2)
                iters += 1
                accepted = True
                break
            lam = lam * nu
            nu = nu * 2
        if not accepted:
            status = 1
            break
    out.update(poses=poses, points=X, obs_chi2=edges(R, t, X, of, op, px, f, cx, cy, delta)[2], final_chi=cur,
               iterations=iters, status=status)
    return out


def robust_chi(cam, poses, points, obs_frame, obs_point, obs_px, delta):
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    return float(edges(rotmat(poses[:, :4]), poses[:, 4:], np.asarray(points, np.float64), np.asarray(obs_frame),
                       np.asarray(obs_point), np.asarray(obs_px, np.float64), cam["fx"], cam["cx"], cam["cy"], delta)[4].sum())


# ---------------------------------------------------------------- scenes
class Scene:
    """One synthetic problem: KITTI camera, depths 6-40 m, 0.3 px pixel noise.  poses / points are the perturbed start,
    true_poses / true_points the scene; the observations are grouped by point, points ascending."""

    def __init__(self, seed, n_frames, n_fixed, n_points, obs_min=None, obs_max=None, noise=0.3, outliers=0.0,
                 pose_sigma=(0.02, 0.002), point_sigma=0.02, delta=2.0, structure_iterations=0, max_iterations=10):
        rng = np.random.default_rng(seed)
        cam = KITTI
        self.cam, self.delta = cam, delta
        self.structure_iterations, self.max_iterations = structure_iterations, max_iterations
        F = n_frames
        obs_min = F if obs_min is None else obs_min
        obs_max = F if obs_max is None else obs_max
        true = np.zeros((F, 7))
        for i in range(F):  # a camera moving sideways and forward, turning a little
            centre = np.array([0.25 * i, 0.02 * np.sin(i), 0.12 * i])
            om = np.array([0.004 * np.sin(0.7 * i), 0.01 * i, 0.003 * np.cos(i)])
            T = se3_exp(np.concatenate([np.zeros(3), om]))
            T[4:] = -rotmat(T[:4]) @ centre
            true[i] = T
        px0 = np.stack([rng.uniform(150, cam["width"] - 150, n_points), rng.uniform(60, cam["height"] - 60, n_points)], 1)
        depth = rng.uniform(6.0, 40.0, n_points)
        mid = true[F // 2]
        pc = np.stack([(px0[:, 0] - cam["cx"]) / cam["fx"] * depth, (px0[:, 1] - cam["cy"]) / cam["fx"] * depth, depth], 1)
        Xw = (pc - mid[4:]) @ rotmat(mid[:4])  # R^T (pc - t)
        of, op = [], []
        for j in range(n_points):
            k = int(rng.integers(obs_min, obs_max + 1))
            fr = np.sort(rng.choice(F, size=k, replace=False))
            of += list(fr)
            op += [j] * k
        self.obs_frame = np.array(of, np.int32)
        self.obs_point = np.array(op, np.int32)
        M = len(of)
        R, t = rotmat(true[:, :4]), true[:, 4:]
        c = np.einsum("mij,mj->mi", R[self.obs_frame], Xw[self.obs_point]) + t[self.obs_frame]
        px = np.stack([cam["fx"] * c[:, 0] / c[:, 2] + cam["cx"], cam["fx"] * c[:, 1] / c[:, 2] + cam["cy"]], 1)
        px += noise * rng.standard_normal((M, 2))
        if outliers > 0:
            bad = rng.random(M) < outliers
            px[bad] += 8.0 * rng.standard_normal((int(bad.sum()), 2))
        self.obs_px = px
        self.fixed = np.zeros(F, np.uint8)
        self.fixed[:n_fixed] = 1
        start = true.copy()
        for i in range(n_fixed, F):
            d = np.concatenate([pose_sigma[0] * rng.standard_normal(3), pose_sigma[1] * rng.standard_normal(3)])
            start[i] = se3_compose(se3_exp(d), true[i])
        self.true_poses, self.true_points = true, Xw
        self.poses = start
        self.points = Xw * (1 + point_sigma * rng.standard_normal((n_points, 1)))

    def run(self, dtype=np.float64, reverse=False, **kw):
        s = slice(None, None, -1) if reverse else slice(None)
        args = dict(max_iterations=self.max_iterations, structure_iterations=self.structure_iterations)
        args.update(kw)
        r = bundle_adjust(self.cam, self.poses, self.fixed, self.points, self.obs_frame[s], self.obs_point[s],
                          self.obs_px[s], self.delta, dtype=dtype, **args)
        r["obs_chi2"] = r["obs_chi2"][s]
        return r


@functools.lru_cache(maxsize=None)
def reference(scene_key, dtype_name="float64", reverse=False):
    """The restatement's result for SCENES[scene_key], computed once per process and not to be modified."""
    return SCENES[scene_key]().run(np.dtype(dtype_name).type, reverse)


@functools.lru_cache(maxsize=None)
def scene(scene_key):
    return SCENES[scene_key]()


# the committed scenes.  Two-view: one fixed and one free frame at the lane / wave / workgroup boundaries; local: all
# free (gauge-free, the damping alone regularises) and the 16-frame maximum with 4 fixed; pure structure.
SCENES = {
    # (one and two points on one free frame fit exactly: chi falls below the 1e-3 in the gain ratio's denominator
    # after 2 and 3 iterations, and r with it; these two scenes stop there so that no decision is borderline)
    "tv1": lambda: Scene(101, 2, 1, 1, max_iterations=2),
    "tv2": lambda: Scene(102, 2, 1, 2, max_iterations=3),
    "tv63": lambda: Scene(103, 2, 1, 63),
    "tv64": lambda: Scene(104, 2, 1, 64),
    "tv65": lambda: Scene(105, 2, 1, 65, outliers=0.05),
    "tv257": lambda: Scene(106, 2, 1, 257, outliers=0.05),
    "loc3": lambda: Scene(107, 3, 0, 40, 2, 3, structure_iterations=10),
    # seed 239: the first of seeds 200..259 whose trace holds rejected trials (10 of them) with every |r| >= 0.27
    "loc3r": lambda: Scene(239, 3, 0, 40, 2, 3, pose_sigma=(0.3, 0.03), point_sigma=0.1, structure_iterations=10),
    "loc8": lambda: Scene(108, 8, 0, 80, 2, 8, outliers=0.05, structure_iterations=10),
    "loc16": lambda: Scene(109, 16, 4, 120, 2, 16, outliers=0.05, structure_iterations=10),
    "struct": lambda: Scene(110, 5, 5, 70, 2, 5, outliers=0.05, structure_iterations=10),
}
