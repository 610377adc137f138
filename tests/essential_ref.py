"""numpy restatement of the essential-matrix RANSAC contract (include/svo_c.h, "essential-matrix RANSAC"), written from
that text and independently of the product's code: the counter-based sampler in Python integers, a five-point solver
that takes the null space from numpy's SVD (or, as a second opinion, from `eigh` of the Gram matrix), finds the roots
with the eigenvectors of the 10 x 10 action matrix (numpy `eig`) and polishes them by Gauss-Newton on the ten cubics
in their coefficient form, the Sampson test in the stated operation order, and the sequential stopping rule.

Scenes come from two_view_ref.make_scene with a stated share of the matches displaced by uniform +-40 px.
"""
import functools
import itertools
import math
import sys

import numpy as np

import two_view_ref as T
from common import KITTI

MASK64 = (1 << 64) - 1
RESIDUAL_MAX = 1e-9
DUPLICATE = 1e-6
POLISH_MAX = 10
CLEAR = 1e-5          # a sample is clear when no complex root is this close to real and no two real roots this close
DBL_MIN = sys.float_info.min


# ------------------------------------------------------------------ sampling
def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed, p, h, n):
    """The five distinct indices of sample h of pair p among n matches, or None."""
    idx = []
    for c in range(256):
        r = mix((seed ^ (p << 44) ^ (h << 8) ^ c) & MASK64)
        v = ((r >> 32) * n) >> 32
        if v in idx:
            continue
        idx.append(v)
        if len(idx) == 5:
            return idx
    return None


# ------------------------------------------------------------------ scoring
def normalise(px, cam=KITTI):
    p = np.asarray(px, np.float64).astype(np.float32).astype(np.float64)
    return np.stack([(p[:, 0] - cam["cx"]) / cam["fx"], (p[:, 1] - cam["cy"]) / cam["fy"]], axis=1)


def thr2_of(threshold, cam=KITTI):
    thr = threshold / ((cam["fx"] + cam["fy"]) / 2.0)
    return thr * thr


def sampson_err(E, x1, x2):
    """err of every match for one model (3, 3): each product and sum one rounded operation, in the stated order."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        a = [(E[i, 0] * x1[:, 0] + E[i, 1] * x1[:, 1]) + E[i, 2] for i in range(3)]
        b = [(E[0, j] * x2[:, 0] + E[1, j] * x2[:, 1]) + E[2, j] for j in range(2)]
        num = (x2[:, 0] * a[0] + x2[:, 1] * a[1]) + a[2]
        den = ((a[0] * a[0] + a[1] * a[1]) + b[0] * b[0]) + b[1] * b[1]
        return (num * num) / den


def inliers(E, x1, x2, thr2):
    with np.errstate(invalid="ignore"):
        return sampson_err(E, x1, x2) <= thr2  # False for a NaN


# ------------------------------------------------------------------ five-point solver
# monomials of degree <= 3 in (x, y, z), as exponent triples; the ten of degree 3 first (the ones eliminated)
_LEFT = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_MONO = _LEFT + _BASIS
_EXP = np.array(_MONO)
# (a, b, c) in {x, y, z, 1}^3 -> monomial index
_OF = np.zeros((4, 4, 4), np.int64)
for _a, _b, _c in itertools.product(range(4), repeat=3):
    _e = [0, 0, 0]
    for _v in (_a, _b, _c):
        if _v < 3:
            _e[_v] += 1
    _OF[_a, _b, _c] = _MONO.index(tuple(_e))
_EPS = np.zeros((3, 3, 3))
for _i, _j, _k in itertools.permutations(range(3)):
    _EPS[_i, _j, _k] = np.linalg.det(np.eye(3)[[_i, _j, _k]])


def null_space(x1, x2, method="svd"):
    """(4, 3, 3): an orthonormal basis of the E with x2^T E x1 = 0 for the five matches."""
    h1 = np.concatenate([x1, np.ones((5, 1))], axis=1)
    h2 = np.concatenate([x2, np.ones((5, 1))], axis=1)
    Q = np.einsum("ki,kj->kij", h2, h1).reshape(5, 9)
    if method == "svd":
        return np.linalg.svd(Q)[2][5:].reshape(4, 3, 3)
    w, v = np.linalg.eigh(Q.T @ Q)
    return v[:, :4].T.reshape(4, 3, 3)


def cubics(B):
    """The ten constraints as a 10 x 20 coefficient matrix over _MONO: rows 3i+j of E E^T E - tr(E E^T) E / 2, then
    det E, for E = x B0 + y B1 + z B2 + B3."""
    t = np.einsum("aik,blk,clj->ijabc", B, B, B) - 0.5 * np.einsum("akl,bkl,cij->ijabc", B, B, B)
    d = np.einsum("ijk,ai,bj,ck->abc", _EPS, B[:, 0], B[:, 1], B[:, 2])
    M = np.zeros((10, 20))
    flat = _OF.ravel()
    for r in range(9):
        np.add.at(M[r], flat, t[r // 3, r % 3].ravel())
    np.add.at(M[9], flat, d.ravel())
    return M


def monomials(x, y, z):
    return x ** _EXP[:, 0] * y ** _EXP[:, 1] * z ** _EXP[:, 2]


def d_monomials(x, y, z):
    v = np.array([x, y, z])
    out = np.zeros((20, 3))
    for k in range(3):
        e = _EXP.copy()
        f = e[:, k].astype(np.float64)
        e[:, k] = np.maximum(e[:, k] - 1, 0)
        out[:, k] = f * np.prod(v[None, :] ** e, axis=1)
    return out


def scaled_residual(M, B, s):
    c = M @ monomials(*s)
    E = s[0] * B[0] + s[1] * B[1] + s[2] * B[2] + B[3]
    return float(np.linalg.norm(c) / np.linalg.norm(E) ** 3), c


def polish(M, B, s):
    """Gauss-Newton on the ten cubics from s = (x, y, z): steps while the scaled residual decreases, at most
    POLISH_MAX.  Returns (s, scaled residual)."""
    s = np.array(s, np.float64)
    best, prev = 0.0, s
    for it in itertools.count():
        with np.errstate(all="ignore"):
            rho, c = scaled_residual(M, B, s)
        if it > 0 and not rho < best:
            return prev, best
        best = rho
        if it == POLISH_MAX or rho == 0.0:
            return s, best
        J = M @ d_monomials(*s)
        try:
            step = np.linalg.lstsq(J, c, rcond=None)[0]
        except np.linalg.LinAlgError:
            return s, best
        prev, s = s, s - step


class Sample:
    """models (k, 3, 3) of unit Frobenius norm, clear (bool), residuals (k,), epipolar (k,): the largest
    |x2^T E x1| over the five matches."""


def five_point(x1, x2, method="svd"):
    out = Sample()
    out.models = np.zeros((0, 3, 3))
    out.residuals = np.zeros(0)
    out.epipolar = np.zeros(0)
    out.clear = True
    B = null_space(x1, x2, method)
    M = cubics(B)
    try:
        R = np.linalg.solve(M[:, :10], M[:, 10:])  # the eliminated monomials = -R basis
    except np.linalg.LinAlgError:
        out.clear = False
        return out
    A = np.zeros((10, 10))  # multiplication by x on the basis x^2 xy xz y^2 yz z^2 x y z 1
    A[:6] = -R[:6]          # x x^2 = x^3, x xy = x^2y, x xz = x^2z, x y^2 = xy^2, x yz = xyz, x z^2 = xz^2
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1.0  # x x = x^2, x y = xy, x z = xz, x 1 = x
    if not np.isfinite(A).all():
        out.clear = False
        return out
    w, V = np.linalg.eig(A)
    with np.errstate(all="ignore"):
        sols = (V[6:9] / V[9]).T
    real, models, res = [], [], []
    for lam, s in zip(w, sols):
        if not np.isfinite(s).all():
            out.clear = False
            continue
        size = max(1.0, float(np.abs(s).max()))
        if lam.imag != 0.0:
            if np.abs(s.imag).max() < CLEAR * size:
                out.clear = False
            continue
        real.append(s.real)
    for i, j in itertools.combinations(range(len(real)), 2):
        if np.abs(real[i] - real[j]).max() < CLEAR * max(1.0, np.abs(real[i]).max()):
            out.clear = False
    for s in real:
        s, rho = polish(M, B, s)
        if not rho <= RESIDUAL_MAX:
            continue
        E = s[0] * B[0] + s[1] * B[1] + s[2] * B[2] + B[3]
        E = E / np.linalg.norm(E)
        if any(min(np.abs(E - m).max(), np.abs(E + m).max()) < DUPLICATE for m in models):
            continue
        models.append(E)
        res.append(rho)
    if models:
        out.models = np.stack(models)
        out.residuals = np.array(res)
        h1 = np.concatenate([x1, np.ones((5, 1))], axis=1)
        h2 = np.concatenate([x2, np.ones((5, 1))], axis=1)
        out.epipolar = np.abs(np.einsum("ki,mij,kj->mk", h2, out.models, h1)).max(axis=1)
    return out


def constraint_residual(E):
    """The scaled residual of the ten constraints at a model (any scale)."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    G = E @ E.T
    c = np.concatenate([(G @ E - 0.5 * np.trace(G) * E).ravel(), [np.linalg.det(E)]])
    return float(np.linalg.norm(c) / np.linalg.norm(E) ** 3)


def match_models(a, b):
    """The largest entry difference between two sets of unit models matched up to sign and order (greedy on the
    closest pairs), or inf when their sizes differ."""
    a, b = np.asarray(a).reshape(-1, 9), np.asarray(b).reshape(-1, 9)
    if len(a) != len(b):
        return math.inf
    if len(a) == 0:
        return 0.0
    d = np.minimum(np.abs(a[:, None] - b[None]).max(axis=2), np.abs(a[:, None] + b[None]).max(axis=2))
    worst, used = 0.0, set()
    for i in np.argsort(d.min(axis=1)):
        j = min((j for j in range(len(b)) if j not in used), key=lambda j: d[i, j])
        used.add(j)
        worst = max(worst, float(d[i, j]))
    return worst


# ------------------------------------------------------------------ the stopping rule
def update_iterations(confidence, ep, max_it):
    """(niters, the real quotient or None)."""
    num = max(1.0 - confidence, DBL_MIN)
    den = 1.0 - (1.0 - ep) ** 5
    if den < DBL_MIN:
        return 0, None
    ln, ld = math.log(num), math.log(den)
    if ld >= 0.0 or -ln >= max_it * (-ld):
        return max_it, None
    q = ln / ld
    return int(np.rint(q)), q


def walk(counts, n, confidence, max_it):
    """The sequential rule over counts (H, 10) (H >= the stop): (iterations, best (h, k), n_inliers, diagnostics)."""
    best, win, niters, h = 0, (-1, -1), max_it, 0
    half, ties = math.inf, 0
    while h < niters:
        rose = False
        for k in range(10):
            if counts[h][k] > best:
                best, win, rose = int(counts[h][k]), (h, k), True
        if rose:
            ties += int(np.count_nonzero(np.asarray(counts[h]) == best)) > 1
            niters, q = update_iterations(confidence, (n - best) / n, max_it)
            if q is not None:
                half = min(half, abs(abs(q - math.floor(q)) - 0.5))
        h += 1
    return h, win, best, {"half_integer_margin": half, "ties": ties}


class Run:
    pass


def ransac(ref_px, cur_px, threshold=1.0, confidence=0.999, max_iterations=1000, seed=0, pair=0, cam=KITTI,
           method="svd"):
    """The whole contract for one pair (whose index enters the sampler)."""
    r = Run()
    n = len(ref_px)
    x1, x2 = normalise(ref_px, cam), normalise(cur_px, cam)
    thr2 = thr2_of(threshold, cam)
    r.samples, r.counts = [], []
    r.E, r.mask = np.zeros((3, 3)), np.zeros(n, np.uint8)
    r.n_inliers, r.iterations, r.best, r.status = 0, 0, (-1, -1), -1
    r.margin = math.inf  # the smallest |err / thr2 - 1| over every decision up to the stop
    if n < 5:
        r.diag = {"half_integer_margin": math.inf, "ties": 0}
        return r
    best, win, niters, h = 0, (-1, -1), max_iterations, 0
    half, ties = math.inf, 0
    while h < niters:
        idx = sample(seed, pair, h, n)
        s = five_point(x1[idx], x2[idx], method) if idx is not None else None
        row = np.full(10, -1, np.int64)
        if s is not None:
            for k, E in enumerate(s.models):
                err = sampson_err(E, x1, x2)
                with np.errstate(all="ignore"):
                    row[k] = int(np.count_nonzero(err <= thr2))
                    m = np.abs(err / thr2 - 1.0)
                r.margin = min(r.margin, float(np.nanmin(m)))
        r.samples.append(s)
        r.counts.append(row)
        rose = False
        for k in range(10):
            if row[k] > best:
                best, win, rose = int(row[k]), (h, k), True
        if rose:
            ties += int(np.count_nonzero(row == best)) > 1
            niters, q = update_iterations(confidence, (n - best) / n, max_iterations)
            if q is not None:
                half = min(half, abs(abs(q - math.floor(q)) - 0.5))
        h += 1
    r.iterations, r.best, r.n_inliers = h, win, best
    r.diag = {"half_integer_margin": half, "ties": ties}
    r.counts = np.array(r.counts).reshape(-1, 10)
    if best > 0:
        r.status = 0
        r.E = r.samples[win[0]].models[win[1]]
        r.mask = inliers(r.E, x1, x2, thr2).astype(np.uint8)
    return r


# ------------------------------------------------------------------ scenes
def with_outliers(s, share, seed):
    """A share of the matches' current pixels displaced by uniform +-40 px (at least 5 px away); s.inlier marks the
    rest."""
    rng = np.random.default_rng(seed)
    n = s.n
    k = int(round(share * n))
    out = rng.permutation(n)[:k]
    d = rng.uniform(-40.0, 40.0, (k, 2))
    d[np.abs(d).max(axis=1) < 5.0] += 7.0
    s.cur_px = s.cur_px.copy()
    s.cur_px[out] += d
    s.inlier = np.ones(n, bool)
    s.inlier[out] = False
    return s


def planar_scene(seed, n, cam=KITTI):
    """make_scene's motion with every point on one slanted plane (noise-free)."""
    s = T.make_scene(seed, n, "side", noise=0.0, cam=cam)
    iK, K = T.invK_of(cam), T.K_of(cam)
    rays = (iK @ np.concatenate([s.ref_px, np.ones((n, 1))], axis=1).T).T
    nrm, d = np.array([0.15, -0.1, 1.0]), 20.0
    Xr = rays * (d / (rays @ nrm))[:, None]
    Xc = Xr @ s.R_true.T + s.t_true
    v = (K @ Xc.T).T
    s.cur_px = np.ascontiguousarray(v[:, :2] / v[:, 2:3])
    s.X_ref_true = Xr
    return s


# the committed scenes: name -> (builder, RANSAC arguments).  Every GPU comparison and every condition of the CPU tests
# runs on these.
def _scene(name):
    kind, n, share, noise, seed = SCENES[name][:5]
    if kind == "planar":
        s = planar_scene(seed, n)
    else:
        s = T.make_scene(seed, n, kind, noise=noise)
    return with_outliers(s, share, seed + 1000)


#        kind     n     outliers noise scene-seed  ransac-seed max_iterations
SCENES = {
    "n5": ("side", 5, 0.0, 0.0, 11, 1, 1000),
    "n6": ("side", 6, 0.0, 0.0, 12, 2, 1000),
    "n63": ("side", 63, 0.3, 0.3, 13, 3, 1000),
    "n64": ("side", 64, 0.3, 0.3, 14, 4, 1000),
    "n65": ("side", 65, 0.3, 0.3, 15, 5, 64),
    "n257": ("side", 257, 0.3, 0.3, 16, 6, 1000),
    "n2000": ("side", 2000, 0.3, 0.3, 17, 7, 1000),
    "one": ("side", 200, 0.3, 0.3, 18, 8, 1),
    "forward": ("forward", 200, 0.2, 0.3, 19, 9, 1000),
    "general": ("side", 200, 0.3, 0.0, 20, 10, 1000),
    "planar": ("planar", 200, 0.3, 0.0, 21, 15, 1000),
    "half": ("side", 200, 0.5, 0.3, 22, 12, 1000),
    "fifth": ("side", 200, 0.2, 0.3, 22, 12, 1000),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return _scene(name)


@functools.lru_cache(maxsize=None)
def scene_run(name, method="svd", pair=0):
    s = scene(name)
    return ransac(s.ref_px, s.cur_px, 1.0, 0.999, SCENES[name][6], SCENES[name][5], pair, method=method)
