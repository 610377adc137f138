"""float64 / int64 numpy restatement of the svo_klt_track contract (include/svo_c.h, "sparse optical flow"), written
from the header text: the derivative images are formed whole per level (np.pad reflect = BORDER_REFLECT_101) and
sampled, all points advance together under masks.  Also the scene makers of tests/test_klt.py.

klt_track() returns positions, status, the per-level trace and a `borderline` flag per point: set when any decision
of that point was close (|minEig - threshold|, |D - FLT_EPSILON| or |delta.delta - eps^2| within 1e-12 relative, an
oscillation test within 1e-12 of 0.01, a floor argument within 1e-9 of an integer), i.e. when a last-bit difference in
the fp64 tail could flip a branch."""
import functools

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
SKIPPED, EPS, OSCILLATION, ITERATION_LIMIT, LEFT_IMAGE, TEMPLATE_OUT, MIN_EIG = range(7)
_S20 = 2.0 ** -20


def pyramid_levels(img, levels):
    """The intensity stack of ImagePyramid::createImagePyramid (level l = cv::pyrDown of level l - 1) as the CPU
    oracle builds it: the planes svo_pyramid_set_build holds."""
    import oracle as O
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    return [p.copy() for p in O.unpack_levels(O.build_pyramid(img, levels)[0], w, h, levels)]


def _refl(i, n):
    i = np.abs(i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def _descale(v, k):
    return (v + (1 << (k - 1))) >> k


def _weights(a, b):
    w00 = np.rint((1.0 - a) * (1.0 - b) * 16384.0).astype(np.int64)
    w01 = np.rint(a * (1.0 - b) * 16384.0).astype(np.int64)
    w10 = np.rint((1.0 - a) * b * 16384.0).astype(np.int64)
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _scharr(img):
    """(Ix, Iy) of the whole plane, int64, REFLECT_101 inside the 3x3."""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    H, W = img.shape

    def s(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ix = 3 * (s(-1, 1) - s(-1, -1)) + 10 * (s(0, 1) - s(0, -1)) + 3 * (s(1, 1) - s(1, -1))
    iy = 3 * (s(1, -1) - s(-1, -1)) + 10 * (s(1, 0) - s(-1, 0)) + 3 * (s(1, 1) - s(-1, 1))
    return ix, iy


def _sample_reflect(img, X, Y):
    H, W = img.shape
    return img[_refl(Y, H), _refl(X, W)].astype(np.int64)


def _sample_zero(der, X, Y):
    H, W = der.shape
    inside = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    return np.where(inside, der[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)], 0)


def _S(sample, plane, X, Y, w):
    w00, w01, w10, w11 = (v[:, None] for v in w)
    return (w00 * sample(plane, X, Y) + w01 * sample(plane, X + 1, Y) + w10 * sample(plane, X, Y + 1) +
            w11 * sample(plane, X + 1, Y + 1))


def _in_range(fx, fy, win, W, H):
    with np.errstate(invalid="ignore"):
        return (fx >= -win) & (fx < W) & (fy >= -win) & (fy < H)


def _near_int(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.rint(x)) < 1e-9


def _rel_close(x, y):
    with np.errstate(invalid="ignore"):
        return np.abs(x - y) <= 1e-12 * np.maximum(np.abs(x), np.abs(y))


def top_level(shapes, win, max_level):
    """Step 2: the largest l <= max_level whose plane is larger than the window on both axes (0 if none)."""
    L = max_level
    while L > 0 and not (shapes[L][1] > win and shapes[L][0] > win):
        L -= 1
    return L


def klt_track(ref_pyr, cur_pyr, ref_px, cur_px, win=11, max_level=3, max_iterations=30, epsilon=1e-4,
              min_eig_threshold=1e-4):
    """ref_pyr / cur_pyr: lists of uint8 planes (level 0 first).  Returns (cur (n, 2) float64, status (n,) uint8,
    trace (n, max_level + 1, 2) int32, borderline (n,) bool)."""
    ref = np.asarray(ref_px, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)   # step 1
    flow = np.asarray(cur_px, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)
    n = len(ref)
    h = (win - 1) // 2
    ky, kx = (v.reshape(-1).astype(np.int64) for v in np.mgrid[0:win, 0:win])
    status = np.ones(n, np.uint8)
    trace = np.zeros((n, max_level + 1, 2), np.int32)
    border = np.zeros(n, bool)
    L = top_level([p.shape for p in ref_pyr], win, max_level)
    flow = flow / float(1 << L)
    for l in range(L, -1, -1):
        if l != L:
            flow = flow * 2.0
        I, J = ref_pyr[l], cur_pyr[l]
        H, W = I.shape
        # step 3
        p = ref / float(1 << l) - h
        fp = np.floor(p)
        border |= _near_int(p).any(axis=1)
        ok = _in_range(fp[:, 0], fp[:, 1], win, W, H)
        trace[~ok, l, 1] = TEMPLATE_OUT
        if l == 0:
            status[~ok] = 0
        idx = np.nonzero(ok)[0]
        if len(idx) == 0:
            continue
        ip = fp[idx].astype(np.int64)
        w = _weights(p[idx, 0] - fp[idx, 0], p[idx, 1] - fp[idx, 1])
        X, Y = ip[:, 0:1] + kx[None, :], ip[:, 1:2] + ky[None, :]
        ix, iy = _scharr(I)
        T = _descale(_S(_sample_reflect, I, X, Y, w), 9)
        gx = _descale(_S(_sample_zero, ix, X, Y, w), 14)
        gy = _descale(_S(_sample_zero, iy, X, Y, w), 14)
        # step 4
        A11 = (gx * gx).sum(axis=1).astype(np.float64) * _S20
        A12 = (gx * gy).sum(axis=1).astype(np.float64) * _S20
        A22 = (gy * gy).sum(axis=1).astype(np.float64) * _S20
        D = A11 * A22 - A12 * A12
        df = A11 - A22
        min_eig = (A22 + A11 - np.sqrt(df * df + 4.0 * A12 * A12)) / float(2 * win * win)
        border[idx] |= _rel_close(min_eig, min_eig_threshold) | _rel_close(D, FLT_EPSILON)
        rej = (min_eig < min_eig_threshold) | (D < FLT_EPSILON)
        trace[idx[rej], l, 1] = MIN_EIG
        if l == 0:
            status[idx[rej]] = 0
        keep = ~rej
        idx, T, gx, gy, A11, A12, A22, D = (v[keep] for v in (idx, T, gx, gy, A11, A12, A22, D))
        if len(idx) == 0:
            continue
        # step 5
        m = len(idx)
        with np.errstate(divide="ignore"):
            invD = 1.0 / D
        q = flow[idx] - h
        prev = np.zeros((m, 2))
        code = np.full(m, ITERATION_LIMIT, np.int32)
        iters = np.zeros(m, np.int32)
        live = np.ones(m, bool)
        eps2 = epsilon * epsilon
        for j in range(max_iterations):
            a = np.nonzero(live)[0]
            if len(a) == 0:
                break
            fq = np.floor(q[a])
            border[idx[a]] |= _near_int(q[a]).any(axis=1)
            inr = _in_range(fq[:, 0], fq[:, 1], win, W, H)
            code[a[~inr]] = LEFT_IMAGE
            live[a[~inr]] = False
            a, fq = a[inr], fq[inr]
            if len(a) == 0:
                break
            iq = fq.astype(np.int64)
            wq = _weights(q[a, 0] - fq[:, 0], q[a, 1] - fq[:, 1])
            Xq, Yq = iq[:, 0:1] + kx[None, :], iq[:, 1:2] + ky[None, :]
            d = _descale(_S(_sample_reflect, J, Xq, Yq, wq), 9) - T[a]
            b1 = (d * gx[a]).sum(axis=1).astype(np.float64) * _S20
            b2 = (d * gy[a]).sum(axis=1).astype(np.float64) * _S20
            dx = (A12[a] * b2 - A22[a] * b1) * invD[a]
            dy = (A12[a] * b1 - A11[a] * b2) * invD[a]
            q[a, 0] += dx
            q[a, 1] += dy
            iters[a] = j + 1
            dd = dx * dx + dy * dy
            border[idx[a]] |= _rel_close(dd, eps2)
            conv = dd <= eps2
            sx, sy = np.abs(dx + prev[a, 0]), np.abs(dy + prev[a, 1])
            if j > 0:
                border[idx[a]] |= ~conv & ((np.abs(sx - 0.01) < 1e-12) | (np.abs(sy - 0.01) < 1e-12))
                osc = ~conv & (sx < 0.01) & (sy < 0.01)
            else:
                osc = np.zeros(len(a), bool)
            q[a[osc], 0] -= dx[osc] * 0.5
            q[a[osc], 1] -= dy[osc] * 0.5
            code[a[conv]] = EPS
            code[a[osc]] = OSCILLATION
            live[a[conv | osc]] = False
            prev[a, 0], prev[a, 1] = dx, dy
        flow[idx] = q + h
        trace[idx, l, 0] = iters
        trace[idx, l, 1] = code
        if l == 0:
            status[idx[code == LEFT_IMAGE]] = 0
    out = flow.astype(np.float32).astype(np.float64)  # step 6
    return out, status, trace, border


# ---------------------------------------------------------------- scenes
class Texture:
    """Band-limited texture: a sum of n_waves sinusoids of 0.01 - 0.12 cycles / px in random directions, evaluated
    analytically, so a shifted view needs no interpolation: render(w, h, shift) is the image whose content moved by
    `shift` (a feature at p in render(w, h) lies at p + shift there)."""

    def __init__(self, seed, n_waves=40):
        rng = np.random.default_rng(seed)
        f = rng.uniform(0.01, 0.12, n_waves)
        th = rng.uniform(0.0, 2.0 * np.pi, n_waves)
        self.fx, self.fy = f * np.cos(th), f * np.sin(th)
        self.ph = rng.uniform(0.0, 2.0 * np.pi, n_waves)
        self.amp = rng.uniform(0.5, 1.0, n_waves) / np.sqrt(f / 0.01)  # more energy in the coarse waves
        self.amp *= 45.0 / np.sqrt(0.5 * (self.amp ** 2).sum())        # standard deviation 45 grey levels

    def render(self, w, h, shift=(0.0, 0.0)):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        x, y = x - shift[0], y - shift[1]
        v = np.full((h, w), 127.5)
        for fx, fy, ph, a in zip(self.fx, self.fy, self.ph, self.amp):
            v += a * np.sin(2.0 * np.pi * (fx * x + fy * y) + ph)
        return np.rint(np.clip(v, 0.0, 255.0)).astype(np.uint8)


def with_rectangle(img, x0, y0, w, h, value=90):
    """`img` with a constant w x h rectangle at (x0, y0)."""
    out = img.copy()
    out[y0:y0 + h, x0:x0 + w] = value
    return out


RECT = (60, 50, 44, 42)  # x0, y0, w, h of the constant rectangle of the 160 x 120 scenes


def scene_points(w, h, win, n, seed, rect=None):
    """n reference positions (none on the pixel grid at any level): the window crossing each of the four edges, two
    positions more than win outside the frame, the rectangle's centre, then uniform ones over the frame and a margin."""
    rng = np.random.default_rng(seed)
    special = [(2.31, h * 0.5 + 0.43), (w - 2.77, h * 0.4 + 0.19), (w * 0.45 + 0.61, 1.87), (w * 0.6 + 0.27, h - 3.21),
               (-win - 7.41, h * 0.3 + 0.77), (w * 0.5 + 0.13, h + win + 9.29)]
    if rect is not None:
        special.append((rect[0] + rect[2] * 0.5 + 0.37, rect[1] + rect[3] * 0.5 - 0.29))
    pts = np.empty((n, 2))
    k = min(n, len(special))
    pts[:k] = special[:k]
    pts[k:, 0] = rng.uniform(-3.0, w + 3.0, n - k)
    pts[k:, 1] = rng.uniform(-3.0, h + 3.0, n - k)
    return pts


@functools.lru_cache(maxsize=None)
def gpu_scene(name):
    """The committed scenes of the GPU tests: dict(ref_img, cur_img, ref_px, init, win, max_level, max_iterations).
    `init` is the initial flow: the reference positions (what computeOpticalFlowSparse passes) except where noted."""
    shift = (3.3, -2.6)
    if name in ("win5", "win11", "win21", "iter2"):
        win = {"win5": 5, "win11": 11, "win21": 21, "iter2": 11}[name]
        tex = Texture(101)
        ref = with_rectangle(tex.render(160, 120), *RECT)
        cur = with_rectangle(tex.render(160, 120, shift), *RECT)
        px = scene_points(160, 120, win, 257, 7, RECT)
        init = px.copy()
        init[10] = (-40.3, 50.2)      # starts far outside: leaves the image
        init[11] = (px[11, 0] + 400.7, px[11, 1])
        return dict(ref_img=ref, cur_img=cur, ref_px=px, init=init, win=win, max_level=3,
                    max_iterations=2 if name == "iter2" else 30)
    if name == "cut":  # 96 x 64: level 3 is 12 x 8, not larger than the window, so L = 2
        tex = Texture(202)
        px = scene_points(96, 64, 11, 65, 9)
        return dict(ref_img=tex.render(96, 64), cur_img=tex.render(96, 64, (1.7, 1.2)), ref_px=px, init=px.copy(),
                    win=11, max_level=3, max_iterations=30)
    if name == "noisy":  # a non-trivial initial flow: truth + N(0, 1.5 px)
        tex = Texture(303)
        sh = (-5.4, 3.8)
        px = scene_points(160, 120, 11, 90, 11)
        init = px + np.asarray(sh) + np.random.default_rng(12).normal(0.0, 1.5, px.shape)
        return dict(ref_img=tex.render(160, 120), cur_img=tex.render(160, 120, sh), ref_px=px, init=init, win=11,
                    max_level=3, max_iterations=30)
    raise KeyError(name)


GPU_SCENES = ("win5", "win11", "win21", "iter2", "cut", "noisy")


@functools.lru_cache(maxsize=None)
def gpu_scene_reference(name):
    """klt_track of a committed scene on the CPU oracle's pyramids, computed once and shared (treat as read-only)."""
    s = gpu_scene(name)
    levels = s["max_level"] + 1
    out = klt_track(pyramid_levels(s["ref_img"], levels), pyramid_levels(s["cur_img"], levels), s["ref_px"], s["init"],
                    s["win"], s["max_level"], s["max_iterations"])
    for a in out:
        a.setflags(write=False)
    return out
